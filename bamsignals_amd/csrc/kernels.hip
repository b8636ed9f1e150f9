// gfx950 (MI355X, CDNA4) kernels for the bamsignals interval-counting hot path.
//
// Replaces the per-read loop of overlapAndPileup<T> (reference src/bamsignals.cpp:240-291)
// with one workgroup per *tile* of a range: bins staged in LDS, 16-B coalesced loads of the
// read columns, LDS integer atomics for the histogram, 16-B coalesced stores of the result.
// Pure 32-bit integer work, HBM-bound: no MFMA anywhere.
//
//   k_profile   Pileupper::setRead/pileup       src/bamsignals.cpp:326-363  (binsize >= 1)
//   k_count     the same with binsize <= 0      src/bamsignals.cpp:148-169, 349-363
//   k_coverage  Coverager::setRead/pileup+cumsum src/bamsignals.cpp:392-438, 464-470
//   k_coverage_bins  the same summed over bins and / or split by strand (bamCoverage's binsize / ss)
//   k_cigar_end bam_endpos - 1 from packed CIGAR (htslib; call site src/bamsignals.cpp:16-18)
//   k_span_hist / k_scatter / k_build_idx       one-time layout of the reads in HBM (bsig_types.h)
//   k_visits    counts read visits for the roofline figure
#include <hip/hip_runtime.h>
#include <type_traits>
#include <stdint.h>
#include <stdlib.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <string>

#include "bsig_types.h"
#include "kernels.h"

#ifdef BSIG_STAMPS
// Diagnostic build only (libbamsignals_hip_stamps.so, scripts/stamps.py): per-workgroup
// s_memrealtime stamps (100 MHz, one counter for the whole chip) of k_profile's phases.  The shipped library has no stamp code.
__device__ unsigned long long *g_stamp_buf = nullptr;
__device__ int g_ablate = 0;     // bit 0: skip the read streaming; bit 1: skip the global stores
#define BSIG_STAMP(k)                                                                       \
    do {                                                                                    \
        if (g_stamp_buf && threadIdx.x == 0) {                                              \
            unsigned long long t_;                                                          \
            asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");    \
            g_stamp_buf[(size_t)blockIdx.x * 8 + (k)] = t_;                                 \
        }                                                                                   \
    } while (0)
#define BSIG_ABLATE(bit) (g_ablate & (bit))
#else
#define BSIG_STAMP(k) do { } while (0)
#define BSIG_ABLATE(bit) 0
#endif

namespace {

constexpr int kWave = 64;

// ------------------------------------------------------------------------------------------
// shared device helpers
// ------------------------------------------------------------------------------------------

// The filter of Pileupper::setRead (src/bamsignals.cpp:328-333) == Coverager::setRead (:394-399), in two parts:
// what only reads flag and mapq (:328-331) -- a property of the (flag, mapq) pair, evaluated per read for the
// span classes and once per code and launch for the packed class (build_ptab) -- ...
__device__ __forceinline__ bool fm_rejected(const BsigKParams &P, uint32_t fm)
{
    const uint32_t nf = ~(fm & 0xFFFFu);                 // ~flag after int promotion
    const int mapq = (int)((fm >> 16) & 0xFFu);
    return (mapq < P.mapqual) | ((P.requiredF & nf) != 0u) | ((P.filteredF & nf) == 0u);
}
// ... and what reads the template length (:332-333)
// bamCount's whole per-read work without a branch (ref: src/bamsignals.cpp:326-363 with binsize = the range): `acc`
// counts the read in its low half if it is one, passes the filters and has its 5' end in [glo, glo + gn), and in its
// high half too if it lies on the reverse strand (a lane sees at most 32,768 reads of a tile, the heavy-tile ceiling)
__device__ __forceinline__ void count_one(const BsigKParams &P, int glo, int gn, int p, int e, bool neg, bool rej, int tl,
                                          bool valid, uint32_t &acc)
{
    bool ok = valid & !rej;
    int offset = P.shift;
    if (P.has_tlen_filter | P.midpoint) {                  // (uniform)
        const int a = tl < 0 ? -tl : tl;
        if (P.has_tlen_filter) ok = ok & (a >= P.tf0) & (a <= P.tf1);
        if (P.midpoint) offset += a >> 1;
    }
    const int p5 = neg ? e - offset : p + offset;
    ok = ok & ((unsigned)(p5 - glo) < (unsigned)gn);
    acc += ok ? (neg ? 0x10001u : 1u) : 0u;
}

__device__ __forceinline__ bool tlen_rejected(const BsigKParams &P, int32_t tl)
{
    if (!P.has_tlen_filter) return false;
    const int a = tl < 0 ? -tl : tl;
    return (a < P.tf0) | (a > P.tf1);
}

// bamProfile's per-read work (ref: src/bamsignals.cpp:326-363) on a tile image of 16-bit cells, two per LDS dword.
template <bool SS>
struct ProfileOne {
    const BsigKParams &P;
    uint32_t *cnt;
    int loc, len, c0, nc, sh;
    bool neg_range;
    __device__ __forceinline__ void operator()(int p, int e, bool neg /* isNegStrand, :11-13 */, bool rej, int tl, bool valid) const
    {
        constexpr int S = SS ? 2 : 1;
        if (!valid || rej || tlen_rejected(P, tl)) return;             // :328-333
        const int a = tl < 0 ? -tl : tl;
        const int offset = P.midpoint ? (a >> 1) + P.shift : P.shift;  // :339
        const int p5 = neg ? e - offset : p + offset;                  // :340-344
        int rel = p5 - loc;                                            // :351
        if ((unsigned)rel >= (unsigned)len) return;                    // :353
        int anti = neg ? 1 : 0;
        if (neg_range) { rel = len - rel - 1; anti ^= 1; }             // :356-359
        const int cell = P.binsize == 1 ? rel
                                        : (int)(__umulhi((uint32_t)rel, P.div_magic) >> P.div_shift);
        const int lc = cell - c0;
        if ((unsigned)lc < (unsigned)nc) {
            const int k = sh + lc * S + (SS ? anti : 0);               // :361-362
            atomicAdd(&cnt[k >> 1], 1u << ((k & 1) << 4));
        }
    }
    // Four reads of the packed class at once for bins of one base: straight arithmetic on the packed word, one masked LDS add at the end.  With d = (word - base) & mask the 5' end relative to the range is
    // d + cp on the forward strand and d + span + cp - 2 shift on the reverse one; the tile's cell is that minus c0,
    // or counted from the range's other end on a reverse-strand range (a tile lies inside its range, so the cell
    // test is the range test, :351-353).
    __device__ __forceinline__ void quad(const uint4 &w, const int4 &t, uint32_t dj, uint32_t nj, int base,
                                         const uint8_t *__restrict__ ptab) const
    {
        const uint32_t b0 = ptab[w.x >> 23], b1 = ptab[w.y >> 23], b2 = ptab[w.z >> 23], b3 = ptab[w.w >> 23];
        if (P.binsize != 1) {                                          // (uniform)
            auto dec = [&](uint32_t x, uint32_t b, int tl, bool valid) {
                const int pos = base + (int)((x - (uint32_t)base) & (((uint32_t)1 << BSIG_PACK_POS_BITS) - 1u));
                (*this)(pos, pos + (int)((x >> BSIG_PACK_POS_BITS) & 0xFFu), (b & 2u) != 0u, (b & 1u) != 0u, tl, valid);
            };
            dec(w.x, b0, t.x, dj < nj);
            dec(w.y, b1, t.y, dj + 1u < nj);
            dec(w.z, b2, t.z, dj + 2u < nj);
            dec(w.w, b3, t.w, dj + 3u < nj);
            return;
        }
        const bool tl_rule = (P.has_tlen_filter | P.midpoint) != 0;    // (uniform)
        if (neg_range) {
            const int K = len - 1 - c0 - (base - loc + P.shift);
            if (tl_rule) four<true, true>(w, t, b0, b1, b2, b3, dj, nj, base, K);
            else four<true, false>(w, t, b0, b1, b2, b3, dj, nj, base, K);
        } else {
            const int K = base - loc + P.shift - c0;
            if (tl_rule) four<false, true>(w, t, b0, b1, b2, b3, dj, nj, base, K);
            else four<false, false>(w, t, b0, b1, b2, b3, dj, nj, base, K);
        }
    }
    // TL: a template-length rule applies (:332-333 the filter, :339 the midpoint: the 5' end moves by |tlen| / 2)
    template <bool REV, bool TL>
    __device__ __forceinline__ void four(const uint4 &w, const int4 &t, uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3, uint32_t dj,
                                         uint32_t nj, int base, int K) const
    {
        const uint32_t cd = (uint32_t)(-2 * P.shift);
        auto rd = [&](uint32_t x, uint32_t b, int tl, uint32_t k) {
            const uint32_t d = (x - (uint32_t)base) & (((uint32_t)1 << BSIG_PACK_POS_BITS) - 1u);
            const uint32_t sp = (x >> BSIG_PACK_POS_BITS) & 0xFFu;
            const uint32_t nm = (uint32_t)((int32_t)(b << 30) >> 31);
            uint32_t rj = (uint32_t)((int32_t)(b << 31) >> 31), h = 0;
            if (TL) {
                const int a = tl < 0 ? -tl : tl;
                if (P.has_tlen_filter) rj |= ((a < P.tf0) | (a > P.tf1)) ? 0xFFFFFFFFu : 0u;
                if (P.midpoint) h = (uint32_t)(a >> 1);
            }
            // 5' end from base + shift: pos + h on the forward strand, pos + span - 2 shift - h on the reverse one
            const uint32_t fwd = d + h + (nm & (sp + cd - 2u * h));
            const uint32_t lc = (REV ? (uint32_t)K - fwd : (uint32_t)K + fwd) | rj;       // (rejected: beyond every tile)
            const bool ok = (dj + k < nj) & (lc < (uint32_t)nc);
            // antisense: reverse-strand read on a forward range, forward read on a reverse one
            const uint32_t cell = SS ? (uint32_t)sh + 2u * lc + ((REV ? ~nm : nm) & 1u) : (uint32_t)sh + lc;
            // (masked, not redirected: the many reads of a window that miss the tile would all meet in one dummy
            // cell, and LDS atomics on one address take their turns -- config 5's 1-kb tiles: 0.16 -> 0.30 ms)
            if (ok) atomicAdd(&cnt[cell >> 1], 1u << ((cell << 4) & 31u));     // (odd cell: the dword's high half)
        };
        rd(w.x, b0, t.x, 0u);
        rd(w.y, b1, t.y, 1u);
        rd(w.z, b2, t.z, 2u);
        rd(w.w, b3, t.w, 3u);
    }
    // Eight reads of the packed class from its 16-bit column p5h (BsigKParams::packed_half: bins of one base, no
    // template-length rule, no code rejected, the window one chunk).  A half-word h holds the low 15 bits of the
    // 5' end and the strand in bit 15: d = (h - base) & 0x7FFF is the 5' end's distance from base, exact because
    // bsig_plan_create keeps every window 256 bases short of a chunk.  No filter table, no span.
    __device__ __forceinline__ void oct(const uint4 &w, uint32_t dj, uint32_t nj, int base) const
    {
        if (neg_range) eight<true>(w, dj, nj, base, len - 1 - c0 - (base - loc + P.shift));
        else eight<false>(w, dj, nj, base, base - loc + P.shift - c0);
    }
    template <bool REV>
    __device__ __forceinline__ void eight(const uint4 &w, uint32_t dj, uint32_t nj, int base, int K) const
    {
        const uint32_t cd = (uint32_t)(-2 * P.shift);
        auto rd = [&](uint32_t h, uint32_t k) {                       // h: the half-word in the low 16 bits
            const uint32_t d = (h - (uint32_t)base) & (((uint32_t)1 << BSIG_PACK_POS_BITS) - 1u);
            const uint32_t nm = (uint32_t)((int32_t)(h << 16) >> 31);
            // 5' end from base + shift: d on the forward strand, d - 2 shift on the reverse one (d counts from pos + span - 1)
            const uint32_t fwd = d + (nm & cd);
            const uint32_t lc = REV ? (uint32_t)K - fwd : (uint32_t)K + fwd;
            const bool ok = (dj + k < nj) & (lc < (uint32_t)nc);
            const uint32_t cell = SS ? (uint32_t)sh + 2u * lc + ((REV ? ~nm : nm) & 1u) : (uint32_t)sh + lc;
            if (ok) atomicAdd(&cnt[cell >> 1], 1u << ((cell << 4) & 31u));     // (masked: see four)
        };
        rd(w.x & 0xFFFFu, 0u); rd(w.x >> 16, 1u);
        rd(w.y & 0xFFFFu, 2u); rd(w.y >> 16, 3u);
        rd(w.z & 0xFFFFu, 4u); rd(w.z >> 16, 5u);
        rd(w.w & 0xFFFFu, 6u); rd(w.w >> 16, 7u);
    }
    // Classes 0 and 1 under BsigKParams::short_half have a 16-bit column of the same format, and their windows obey
    // the same bound with the class's own maxspan and bucket (bsig_plan_create).  Their chunk starts where the class's
    // bucket-rounded window of this tile starts -- load_windows' wlo, from the work item alone (scalar arithmetic; a
    // slice of a heavy tile keeps its tile's cells, so its reads lie in the same window).
    __device__ __forceinline__ int short_base(int c) const
    {
        const int64_t b = (int64_t)c0 + nc < len ? (int64_t)c0 + nc : len;                     // (tile_interval, bins of one base)
        const int64_t tlo = neg_range ? (int64_t)loc + len - b : (int64_t)loc + c0;
        const uint32_t sw = (uint32_t)P.short_win[c];                    // ext + maxspan - 1 and the bucket's log2 in one word
        const int64_t wlo = tlo - (int64_t)(sw >> 5);
        return wlo > 0 ? (int)((wlo >> (sw & 31u)) << (sw & 31u)) : 0;
    }
    // ... and a window of at most one read per lane takes `eight`'s rd for the lane's one half-word h (valid: the
    // lane has a read)
    __device__ __forceinline__ void half1(uint32_t h, bool valid, int base) const
    {
        const uint32_t d = (h - (uint32_t)base) & (((uint32_t)1 << BSIG_PACK_POS_BITS) - 1u);
        const uint32_t nm = (uint32_t)((int32_t)(h << 16) >> 31);
        const uint32_t fwd = d + (nm & (uint32_t)(-2 * P.shift));
        const uint32_t K = (uint32_t)(neg_range ? len - 1 - c0 - (base - loc + P.shift) : base - loc + P.shift - c0);
        const uint32_t lc = neg_range ? K - fwd : K + fwd;
        const bool ok = valid & (lc < (uint32_t)nc);
        const uint32_t cell = SS ? (uint32_t)sh + 2u * lc + ((neg_range ? ~nm : nm) & 1u) : (uint32_t)sh + lc;
        if (ok) atomicAdd(&cnt[cell >> 1], 1u << ((cell << 4) & 31u));         // (masked: see four)
    }
};

// bamProfile's per-read work on the wide-bin image of k_profile_small: 32-bit cells in the lane's own replica.
template <bool SS>
struct SmallOne {
    const BsigKParams &P;
    int32_t *mine;
    int loc, len, c0, nc;
    bool neg_range;
    __device__ __forceinline__ void operator()(int p, int e, bool neg, bool rej, int tl, bool valid) const
    {
        constexpr int S = SS ? 2 : 1;
        if (!valid || rej || tlen_rejected(P, tl)) return;
        const int a = tl < 0 ? -tl : tl;
        const int offset = P.midpoint ? (a >> 1) + P.shift : P.shift;
        const int p5 = neg ? e - offset : p + offset;
        int rel = p5 - loc;
        if ((unsigned)rel >= (unsigned)len) return;
        int anti = neg ? 1 : 0;
        if (neg_range) { rel = len - rel - 1; anti ^= 1; }
        const int cell = P.binsize == 1 ? rel : (int)(__umulhi((uint32_t)rel, P.div_magic) >> P.div_shift);
        const int lc = cell - c0;
        if ((unsigned)lc < (unsigned)nc) atomicAdd(&mine[lc * S + (SS ? anti : 0)], 1);
    }
    // four packed reads at once, as ProfileOne::quad, with the bin of the range-oriented position by an exact magic
    // multiply.  The launch is bound by its vector instructions (0.98 of it once the replicas were right: `SQ_INSTS_VALU`),
    // so the read body is counted out: the position is taken relative to the TILE's first base (K carries
    // -c0 * binsize), which makes "inside the range" and "one of this tile's cells" ONE unsigned compare against the
    // tile's length in bases and the cell its own index; the table byte is used as it is (bit 0 rejected, bit 1 reverse
    // strand: two v_bfe_i32 make the masks); the strand's half of the address is a mask and an AND; for ranges
    // shorter than 32,768 bases the bin is a 24-bit multiply at the vector unit's full rate instead of the
    // quarter-rate v_mul_hi_u32.  19 vector instructions a read where the round began with 33 and its middle had 26.
    __device__ __forceinline__ void quad(const uint4 &w, const int4 &t, uint32_t dj, uint32_t nj, int base,
                                         const uint8_t *__restrict__ ptab) const
    {
        const uint32_t b0 = ptab[w.x >> 23], b1 = ptab[w.y >> 23], b2 = ptab[w.z >> 23], b3 = ptab[w.w >> 23];
        if (!P.rel24) {                                                // (uniform: shifts or midpoints of megabases)
            auto dec = [&](uint32_t x, uint32_t b, int tl, bool valid) {
                const int pos = base + (int)((x - (uint32_t)base) & (((uint32_t)1 << BSIG_PACK_POS_BITS) - 1u));
                (*this)(pos, pos + (int)((x >> BSIG_PACK_POS_BITS) & 0xFFu), (b & 2u) != 0u, (b & 1u) != 0u, tl, valid);
            };
            dec(w.x, b0, t.x, dj < nj);
            dec(w.y, b1, t.y, dj + 1u < nj);
            dec(w.z, b2, t.z, dj + 2u < nj);
            dec(w.w, b3, t.w, dj + 3u < nj);
            return;
        }
        // (uniform, like everything these branches ask.  Three forms only -- the orientation of the range is a sign and
        // a strand mask, not a fourth template argument: the kernel inlines this at four places, and 32 copies of the
        // read body were 35 KB of code that ran a third SLOWER than round 4's 16)
        const bool tl_rule = (P.has_tlen_filter | P.midpoint) != 0;
        const bool narrow = len < 32768 && P.div_s15 != 0;
        const int A = base - loc + P.shift;
        const int first = c0 * P.binsize;                                  // the tile's first base in range orientation
        const int K = (neg_range ? len - 1 - A : A) - first, sgn = neg_range ? -1 : 1;
        const int rest = len - first, mine_bases = nc * P.binsize;
        const uint32_t tile_bases = (uint32_t)(rest < mine_bases ? rest : mine_bases);
        if (tl_rule) four<true, false>(w, t, b0, b1, b2, b3, dj, nj, base, K, sgn, tile_bases);
        else if (narrow) four<false, true>(w, t, b0, b1, b2, b3, dj, nj, base, K, sgn, tile_bases);
        else four<false, false>(w, t, b0, b1, b2, b3, dj, nj, base, K, sgn, tile_bases);
    }
    template <bool TL, bool NARROW>
    __device__ __forceinline__ void four(const uint4 &w, const int4 &t, uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3, uint32_t dj,
                                         uint32_t nj, int base, int K, int sgn, uint32_t tile_bases) const
    {
        const int cd = -2 * P.shift;                                   // (binsize > 1 here: bins of one base run k_profile)
        const int flip = sgn < 0 ? -1 : 0;
        int Kv = K;
        asm volatile("" : "+v"(Kv));                                   // (in a vector register once: v_mad_i32_i24 takes one scalar operand)
        char *const image = reinterpret_cast<char *>(mine);
        auto rd = [&](uint32_t x, uint32_t b, int tl, uint32_t k) {
            const int d = (int)((x - (uint32_t)base) & (((uint32_t)1 << BSIG_PACK_POS_BITS) - 1u));
            int spcd = (int)((x >> BSIG_PACK_POS_BITS) & 0xFFu) + cd, h = 0;
            const int rev = __builtin_amdgcn_sbfe((int)b, 1, 1);       // all ones: reverse strand
            int rj = __builtin_amdgcn_sbfe((int)b, 0, 1);              // all ones: rejected by flag / mapq
            if (TL) {
                const int a = tl < 0 ? -tl : tl;
                if (P.has_tlen_filter) rj |= ((a < P.tf0) | (a > P.tf1)) ? -1 : 0;
                if (P.midpoint) { h = a >> 1; spcd -= 2 * h; }
            }
            // (|fwd| <= d + span - 1 + 2 |shift| + h < 2^23 under P.rel24, which quad() asked: see bsig_plan_create)
            const int fwd = (rev & spcd) + d + h;
            const uint32_t rel = (uint32_t)(__mul24(fwd, sgn) + Kv) | (uint32_t)rj;     // from the tile's first base, range orientation
            const uint32_t cell = NARROW ? __umul24(rel, P.div_m15) >> P.div_s15 : __umulhi(rel, P.div_magic) >> P.div_shift;
            const bool ok = (dj + k < nj) & (rel < tile_bases);
            if (ok) atomicAdd(reinterpret_cast<int32_t *>(image + (SS ? (cell << 3) + (uint32_t)((rev ^ flip) & 4) : cell << 2)), 1);
        };
        rd(w.x, b0, t.x, 0u);
        rd(w.y, b1, t.y, 1u);
        rd(w.z, b2, t.z, 2u);
        rd(w.w, b3, t.w, 3u);
    }
};

// The interval [start, end] a read that passed the filter covers (ref: src/bamsignals.cpp:401-413), the one rule of
// CoverOne, CoverBinsOne and CoverWideOne: the read as it lies, [p, e]; under P.tspan (paired.end = "extend") the
// fragment its own tlen gives; under P.frag_len = L (a resized plan: single-end reads resized to the fragment) exactly
// L bases from the 5' end in the read's direction -- forward [p, p + L - 1], reverse [e - L + 1, e].  Nothing is clipped at
// the reference's last base; a reverse fragment's bases below 0 are dropped (no reference has them, so no range may
// show them) and a forward fragment's last base saturates at INT32_MAX (a base no read reaches otherwise), which keeps
// both sums inside int32.  P.tspan and P.frag_len are never both set (check_params).  FRAG is a TEMPLATE flag of the
// functors and of the kernels built on them (k_coverage, k_coverage_bins, k_sum_tiles' coverage kinds; the launch picks
// the instantiation by P.frag_len): the coverage launches are bound by their instructions and their kernels sit at the
// scalar register file's limit, where even a uniform branch a read showed (3 - 9 % of a step, measured), so the forms
// without the flag are, instruction for instruction, what they were before the rule existed.
template <bool FRAG>
__device__ __forceinline__ void covered_interval(const BsigKParams &P, int p, int e, bool neg, int tl, int &start, int &end)
{
    start = p; end = e;                                           // :401-403
    if constexpr (FRAG) {
        const int l1 = P.frag_len - 1;
        if (neg) { const int floor0 = e < 0 ? e : 0, s = e - l1; start = s > floor0 ? s : floor0; }
        else end = p > INT32_MAX - l1 ? INT32_MAX : p + l1;
    } else if (P.tspan) {                                         // :404-413
        if (neg && tl < 0) start = end + tl + 1;
        else if (!neg && tl > 0) end = start + tl - 1;
    }
}

// bamCoverage's per-read work (ref: src/bamsignals.cpp:392-438): +1 where the read begins to cover the tile, -1 behind
// its last covered cell, in the tile's difference array of signed 16-bit cells (two per LDS dword: see k_coverage).
template <bool FRAG>
struct CoverOneT {
    const BsigKParams &P;
    int32_t *lds;
    int loc, c0, nc, sh;
    bool neg_range;
    int rend1;                              // last base of the range
    __device__ __forceinline__ void operator()(int p, int e, bool neg, bool rej, int tl, bool valid) const
    {
        if (!valid || rej || tlen_rejected(P, tl)) return;            // :394-399
        int start, end;
        covered_interval<FRAG>(P, p, e, neg, tl, start, end);        // :401-413
        // covered cells [ra, rb] in range orientation (:423-436), then relative to the tile
        const int ra = neg_range ? rend1 - end : start - loc;
        const int rb = neg_range ? rend1 - start : end - loc;
        const int la = ra - c0, lb = rb - c0;
        if (la >= nc || lb < 0) return;                               // :420
        const int ka = sh + (la > 0 ? la : 0);
        atomicAdd(&lds[ka >> 1], (ka & 1) ? 65536 : 1);
        if (lb + 1 < nc) {
            const int kb = sh + lb + 1;
            atomicAdd(&lds[kb >> 1], (kb & 1) ? -65536 : -1);
        }
    }
    // Four reads of the packed class at once (the launch is bound by its vector instructions: PMC, config 3).
    // Straight arithmetic on the packed word -- first covered cell
    // la = d + A (or B - d - span on a reverse-strand range), last lb = la + span, d = (word - base) & mask -- and two
    // masked LDS adds at the end.
    __device__ __forceinline__ void quad(const uint4 &w, const int4 &t, uint32_t dj, uint32_t nj, int base,
                                         const uint8_t *__restrict__ ptab) const
    {
        const uint32_t b0 = ptab[w.x >> 23], b1 = ptab[w.y >> 23], b2 = ptab[w.z >> 23], b3 = ptab[w.w >> 23];
        // (sh rides in K: k = cell index in the image, first covered cell max(ka, sh), one past the last kb)
        const bool tl_rule = (P.has_tlen_filter | P.tspan) != 0;       // (uniform)
        if (neg_range) {
            const int K = rend1 - c0 - base + sh;
            if constexpr (FRAG) four<true, true, true>(w, t, b0, b1, b2, b3, dj, nj, base, K);      // (a resized plan)
            else if (tl_rule) four<true, true>(w, t, b0, b1, b2, b3, dj, nj, base, K);
            else four<true, false>(w, t, b0, b1, b2, b3, dj, nj, base, K);
        } else {
            const int K = base - loc - c0 + sh;
            if constexpr (FRAG) four<false, true, true>(w, t, b0, b1, b2, b3, dj, nj, base, K);
            else if (tl_rule) four<false, true>(w, t, b0, b1, b2, b3, dj, nj, base, K);
            else four<false, false>(w, t, b0, b1, b2, b3, dj, nj, base, K);
        }
    }
    // TL: a template-length rule applies (:398-399 the filter; :404-413 paired.end = "extend": a forward read with
    // tlen > 0 covers tlen bases from its start, a reverse one with tlen < 0 covers -tlen bases up to its end)
    // RESIZE: a resized plan (covered_interval's P.frag_len rule, from the strand bit of the table byte; no tlen is read for
    // it: TL is set with RESIZE only so that a tlen FILTER still applies, under its own uniform flag).  Every term is taken
    // from the chunk's base, and L <= BSIG_FRAG_LEN_MAX = 2^24 keeps each sum below 2^26 (see bsig_plan_create_resized).
    template <bool REV, bool TL, bool RESIZE = false>
    __device__ __forceinline__ void four(const uint4 &w, const int4 &t, uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3, uint32_t dj,
                                         uint32_t nj, int base, int K) const
    {
        const int hi = sh + nc;
        const int l1 = RESIZE ? P.frag_len - 1 : 0;
        auto rd = [&](uint32_t x, uint32_t b, int tl, uint32_t k) {
            const int d = (int)((x - (uint32_t)base) & (((uint32_t)1 << BSIG_PACK_POS_BITS) - 1u));
            const int sp = (int)((x >> BSIG_PACK_POS_BITS) & 0xFFu);
            int rj = (int32_t)(b << 31) >> 31;                             // all ones: rejected
            int s0 = d, e0 = d + sp;                                       // first and last covered base, from `base`
            if (TL) {
                const int a = tl < 0 ? -tl : tl;
                if (P.has_tlen_filter) rj |= ((a < P.tf0) | (a > P.tf1)) ? -1 : 0;
                if (P.tspan) {
                    const int nm = (int32_t)(b << 30) >> 31;               // all ones: reverse strand
                    const int s1 = e0 + tl + 1, e1 = d + tl - 1;
                    s0 = (nm & (tl < 0 ? -1 : 0)) ? s1 : s0;
                    e0 = (~nm & (tl > 0 ? -1 : 0)) ? e1 : e0;
                }
            }
            if (RESIZE) {
                const bool rev = (b & 2u) != 0u;                           // reverse strand
                const int s1 = e0 - l1, floor0 = -base;                    // (a packed read has pos >= 0: base 0 is at -base)
                s0 = rev ? (s1 > floor0 ? s1 : floor0) : s0;
                e0 = rev ? e0 : d + l1;
            }
            const int ka = REV ? K - e0 : K + s0;
            const int kb = ((REV ? K - s0 : K + e0) | rj) + 1;             // (a rejected read ends before the tile)
            const bool ok = (dj + k < nj) & (ka < hi) & (kb > sh);
            const bool ok2 = ok & (kb < hi);
            const int ca = ka > sh ? ka : sh;
            // an odd cell is the high half of its dword: the shifter takes (k << 4) & 31 = 16 for odd k
            // (and -1 is all ones: shifted by 16 it is -65536 in the dword's arithmetic mod 2^32).  The adds are
            // masked, not redirected to a dummy cell: see ProfileOne.
            uint32_t *img = reinterpret_cast<uint32_t *>(lds);
            if (ok) atomicAdd(&img[ca >> 1], 1u << (((uint32_t)ca << 4) & 31u));
            if (ok2) atomicAdd(&img[kb >> 1], 0xFFFFFFFFu << (((uint32_t)kb << 4) & 31u));
        };
        rd(w.x, b0, t.x, 0u);
        rd(w.y, b1, t.y, 1u);
        rd(w.z, b2, t.z, 2u);
        rd(w.w, b3, t.w, 3u);
    }
};
using CoverOne = CoverOneT<false>;

struct CountOne {
    const BsigKParams &P;
    int glo, gn;
    uint32_t &acc;
    __device__ __forceinline__ void operator()(int p, int e, bool neg, bool rej, int tl, bool valid) const
    {
        count_one(P, glo, gn, p, e, neg, rej, tl, valid, acc);
    }
    // four reads of the packed class (words w; read k is one of the window's iff dj + k < nj, unsigned -- not asked
    // at all on an INNER pass, one that lies inside the window with all its reads).  The count family has a table of
    // its own, one DWORD per code (build_ctab: bit 0 reverse strand, bit 31 rejected), which the arithmetic takes as
    // it comes: as a 24-bit factor it is the strand bit, and-ed with the sign bit it is the rejection.  Without a
    // template-length rule the 5' end relative to the interval comes straight out of the word:
    // pos - glo + shift = d + cp and end - glo - shift = d + span + cp + cd with d = (word - base) & mask:
    // rel = d + cp + strand * (span + cd), 13 vector instructions a read (11 on an inner pass; 19 in round 4).
    __device__ __forceinline__ void quad(const uint4 &w, const int4 &t, uint32_t dj, uint32_t nj, int base,
                                         const uint32_t *__restrict__ ctab, bool inner) const
    {
        const uint32_t b0 = ctab[w.x >> 23], b1 = ctab[w.y >> 23], b2 = ctab[w.z >> 23], b3 = ctab[w.w >> 23];
        if (P.has_tlen_filter | P.midpoint | !P.rel24) {      // (uniform; !rel24: shifts of megabases)
            auto dec = [&](uint32_t x, uint32_t b, int tl, bool valid) {
                const int pos = base + (int)((x - (uint32_t)base) & (((uint32_t)1 << BSIG_PACK_POS_BITS) - 1u));
                count_one(P, glo, gn, pos, pos + (int)((x >> BSIG_PACK_POS_BITS) & 0xFFu), (b & 1u) != 0u, (b >> 31) != 0u, tl, valid, acc);
            };
            dec(w.x, b0, t.x, dj < nj);
            dec(w.y, b1, t.y, dj + 1u < nj);
            dec(w.z, b2, t.z, dj + 2u < nj);
            dec(w.w, b3, t.w, dj + 3u < nj);
            return;
        }
        const int cp = base - glo + P.shift, cd = -2 * P.shift;
        auto rel_of = [&](uint32_t x, uint32_t b) {
            const int d = (int)((x - (uint32_t)base) & (((uint32_t)1 << BSIG_PACK_POS_BITS) - 1u));
            const int spcd = (int)((x >> BSIG_PACK_POS_BITS) & 0xFFu) + cd;
            // (|spcd| <= span - 1 + 2 |shift| < 2^23 under P.rel24, asked above: see bsig_plan_create)
            return ((uint32_t)(__mul24((int)b, spcd) + d + cp)) | (b & 0x80000000u);
        };
        if (inner) {
            acc += rel_of(w.x, b0) < (uint32_t)gn ? (b0 << 16 | 1u) : 0u;
            acc += rel_of(w.y, b1) < (uint32_t)gn ? (b1 << 16 | 1u) : 0u;
            acc += rel_of(w.z, b2) < (uint32_t)gn ? (b2 << 16 | 1u) : 0u;
            acc += rel_of(w.w, b3) < (uint32_t)gn ? (b3 << 16 | 1u) : 0u;
        } else {
            acc += ((dj < nj) & (rel_of(w.x, b0) < (uint32_t)gn)) ? (b0 << 16 | 1u) : 0u;
            acc += ((dj + 1u < nj) & (rel_of(w.y, b1) < (uint32_t)gn)) ? (b1 << 16 | 1u) : 0u;
            acc += ((dj + 2u < nj) & (rel_of(w.z, b2) < (uint32_t)gn)) ? (b2 << 16 | 1u) : 0u;
            acc += ((dj + 3u < nj) & (rel_of(w.w, b3) < (uint32_t)gn)) ? (b3 << 16 | 1u) : 0u;
        }
    }
};

// bamOverlaps' per-read work, in count_one's shape (no branch, the same packed counter): a read that passes the filter of
// Coverager::setRead (:394-399) has the interval [s, e] = [pos, end], or CoverOne's fragment under P.tspan (:404-413);
// against the range [lo, hi1] (first and last base) it overlaps in ov = min(e, hi1) - max(s, lo) + 1 bases and counts
// iff ov >= P.minoverlap -- WITHIN: and s >= lo and e <= hi1.  A range wider than one tile is cut into several, and a
// read may overlap more than one: the tile [glo, glo + gn) counts a read iff the read's ANCHOR a = max(s, lo), its
// first base inside the range, lies in the tile.  Every counted read has exactly one anchor tile, so sub-intervals,
// slices of heavy tiles and the shards of several GPUs add up without a read counted twice.
//
// The count-mode window of a tile [tlo, thi) (class_window with ext = tspan ? tf1 : 0: pos in
// [tlo - ext - maxspan + 1, thi + ext)) holds every read anchored in the tile:
//   * a read anchored in [tlo, thi) has e >= a >= tlo; its own end is >= tlo too (a reverse fragment ends with the
//     read, e = end; any other has a in [pos, end]), so pos >= tlo - maxspan + 1 -- and a forward fragment that starts
//     before lo (a = lo = tlo) has pos + tlen - 1 >= lo with tlen <= tf1: pos >= tlo - tf1 + 1;
//   * without a fragment rule pos = s <= a < thi; a forward fragment has pos = s as well;
//   * a reverse fragment has s = end + tlen + 1 <= a < thi, so pos <= end = s - tlen - 1 < thi + tf1.
// glo, gn, lo, hi1 and P.minoverlap are wave-uniform.  No sum here wraps: pos, end and tlen are any int32 and
// tf1 <= 2^30 (bsig_plan_create), so operator() takes a fragment's sums in 64 bits; quad, which sees packed reads only
// (0 <= pos < 2^31, span <= 256, no template length), works in 32 bits relative to its chunk (see there).
template <bool WITHIN>
struct OverlapOne {
    const BsigKParams &P;
    int glo, gn;
    int64_t lo, hi1;
    uint32_t &acc;
    __device__ __forceinline__ void operator()(int p, int e, bool neg, bool rej, int tl, bool valid) const
    {
        bool ok = valid & !rej;
        if (P.has_tlen_filter) {                               // (uniform)
            const int64_t a = tl < 0 ? -(int64_t)tl : (int64_t)tl;
            ok = ok & (a >= P.tf0) & (a <= P.tf1);
        }
        if (!P.tspan) {                                        // (uniform)
            // the read is its own interval: nothing is summed, and 32 bits do.  lo is an int32 (loc); a last base past
            // INT32_MAX is past every e; with b >= a the difference b - a is below 2^32, so the unsigned subtraction
            // is exact; a - glo lies in [-c0, 2^32), so its residue is below gn only where it is itself (a >= lo,
            // glo = lo + c0)
            const int lo32 = (int)lo, hi32 = hi1 > INT32_MAX ? INT32_MAX : (int)hi1;
            const int a = p > lo32 ? p : lo32, b = e < hi32 ? e : hi32;
            ok = ok & (b >= a) & ((uint32_t)b - (uint32_t)a >= (uint32_t)(P.minoverlap - 1)) &
                 ((uint32_t)a - (uint32_t)glo < (uint32_t)gn);
            if (WITHIN) ok = ok & (p >= lo32) & (e <= hi32);
        } else {
            const int64_t s = (neg & (tl < 0)) ? (int64_t)e + tl + 1 : (int64_t)p;
            const int64_t f = (!neg & (tl > 0)) ? (int64_t)p + tl - 1 : (int64_t)e;
            const int64_t a = s > lo ? s : lo, b = f < hi1 ? f : hi1;
            ok = ok & (b - a >= (int64_t)P.minoverlap - 1) & ((uint64_t)(a - glo) < (uint64_t)gn);
            if (WITHIN) ok = ok & (s >= lo) & (f <= hi1);
        }
        acc += ok ? (neg ? 0x10001u : 1u) : 0u;
    }
    // Four reads of the packed class (CountOne::quad's arguments; the table is the overlap forms' own, build_otab: per
    // code what a counted read ADDS to the packed counter -- 1, 0x10001 on the reverse strand, 0 for a rejected code --
    // so the filter and the strand cost no instruction per read).  With a template-length rule they go through operator().  Without one everything is taken from the chunk's start:
    // s = d = (word - base) & mask < 2^15 and e = d + span - 1 < 2^15 + 255, against the range's ends minus `base`,
    // clamped to [-1, 2^20].  The clamps change no answer -- a first base below 0 is below every s, a last base above
    // 2^20 is above every e, a last base below -1 or a first base above 2^20 leaves no overlap either way -- and keep
    // every difference below 2^21 in magnitude.  The anchor test is a subtraction modulo 2^32 of two numbers less than
    // 2^32 apart (0 <= pos < 2^31, glo an int32).  No multiply, so nothing to gate on P.rel24.
    __device__ __forceinline__ void quad(const uint4 &w, const int4 &t, uint32_t dj, uint32_t nj, int base,
                                         const uint32_t *__restrict__ ctab, bool inner) const
    {
        const uint32_t b0 = ctab[w.x >> 23], b1 = ctab[w.y >> 23], b2 = ctab[w.z >> 23], b3 = ctab[w.w >> 23];
        if (P.use_tlen | P.overlap_wide) {                     // (uniform)
            auto dec = [&](uint32_t x, uint32_t b, int tl, bool valid) {
                const int pos = base + (int)((x - (uint32_t)base) & (((uint32_t)1 << BSIG_PACK_POS_BITS) - 1u));
                (*this)(pos, pos + (int)((x >> BSIG_PACK_POS_BITS) & 0xFFu), (b >> 16) != 0u, b == 0u, tl, valid);
            };
            dec(w.x, b0, t.x, dj < nj);
            dec(w.y, b1, t.y, dj + 1u < nj);
            dec(w.z, b2, t.z, dj + 2u < nj);
            dec(w.w, b3, t.w, dj + 3u < nj);
            return;
        }
        auto clamp = [](int64_t v) { return (int)(v < -1 ? -1 : v > (1 << 20) ? (1 << 20) : v); };
        const int lo_b = clamp(lo - base), hi_b = clamp(hi1 - base), m1 = P.minoverlap - 1;
        const uint32_t g_b = (uint32_t)glo - (uint32_t)base;
        auto hit = [&](uint32_t x) {
            const int d = (int)((x - (uint32_t)base) & (((uint32_t)1 << BSIG_PACK_POS_BITS) - 1u));
            const int f = d + (int)((x >> BSIG_PACK_POS_BITS) & 0xFFu);
            const int a = d > lo_b ? d : lo_b, bb = f < hi_b ? f : hi_b;
            bool ok = (bb - a >= m1) & ((uint32_t)a - g_b < (uint32_t)gn);
            if (WITHIN) ok = ok & (d >= lo_b) & (f <= hi_b);
            return ok;
        };
        // (12 vector instructions a read on an inner pass, CountOne's 11: two for d, span, last base, max, min, the two
        // differences and their compares, select, add)
        if (inner) {
            acc += hit(w.x) ? b0 : 0u;
            acc += hit(w.y) ? b1 : 0u;
            acc += hit(w.z) ? b2 : 0u;
            acc += hit(w.w) ? b3 : 0u;
        } else {
            acc += ((dj < nj) & hit(w.x)) ? b0 : 0u;
            acc += ((dj + 1u < nj) & hit(w.y)) ? b1 : 0u;
            acc += ((dj + 2u < nj) & hit(w.z)) ? b2 : 0u;
            acc += ((dj + 3u < nj) & hit(w.w)) ? b3 : 0u;
        }
    }
};

constexpr int kPackChunk = 1 << BSIG_PACK_POS_BITS;        // bases a packed word's position bits span
constexpr uint32_t kPackPosMask = (uint32_t)kPackChunk - 1u;

// Per launch and workgroup: what the flag/mapq filter says about every code of the packed class, one byte per
// code in LDS (bit 0: rejected, bit 1: reverse strand).  The pair table is 2 KB and stays in L2.
// The packed class's filter table (per code: bit 0 rejected by mapq / flag masks, bit 1 reverse strand) depends on
// the file's pair table and the call's parameters only: it is made ONCE PER PLAN (k_make_ptab, 512 bytes on the
// device, BsigKParams::ptab) and every workgroup copies it into its LDS -- one 16-byte load for half the lanes.
// Every workgroup used to build it for itself: 90 vector instructions per wave, 13 % of what a north-star tile
// issues, in launches that are bound by exactly those (NOTES_r04.md, section 9).
template <int NT>
__device__ __forceinline__ void build_ptab(uint8_t *ptab, const BsigReadsDev &R, const BsigKParams &P, int tid)
{
    (void)R;
    const uint4 *src = reinterpret_cast<const uint4 *>(P.ptab);
    uint4 *dst = reinterpret_cast<uint4 *>(ptab);
    for (int v = tid; v < BSIG_PACK_CODES / 16; v += NT) dst[v] = src[v];
}
// ... and the count family's form of it: one dword per code, bit 0 reverse strand, bit 31 rejected (CountOne::quad)
template <int NT>
__device__ __forceinline__ void build_ctab(uint32_t *ctab, const BsigKParams &P, int tid)
{
    const uint32_t *src = reinterpret_cast<const uint32_t *>(P.ptab);
    for (int v = tid; v < BSIG_PACK_CODES / 4; v += NT) {
        const uint32_t b = src[v];
        auto e = [](uint32_t x) { return ((x >> 1) & 1u) | (x << 31); };
        reinterpret_cast<uint4 *>(ctab)[v] = make_uint4(e(b & 0xFFu), e((b >> 8) & 0xFFu), e((b >> 16) & 0xFFu), e(b >> 24));
    }
}
// ... and the overlap forms' (OverlapOne::quad): per code what a counted read adds to the packed counter -- 0 rejected, 1,
// 0x10001 reverse strand
template <int NT>
__device__ __forceinline__ void build_otab(uint32_t *otab, const BsigKParams &P, int tid)
{
    const uint32_t *src = reinterpret_cast<const uint32_t *>(P.ptab);
    for (int v = tid; v < BSIG_PACK_CODES / 4; v += NT) {
        const uint32_t b = src[v];
        auto e = [](uint32_t x) { return (x & 1u) ? 0u : (x & 2u) ? 0x10001u : 1u; };
        reinterpret_cast<uint4 *>(otab)[v] = make_uint4(e(b & 0xFFu), e((b >> 8) & 0xFFu), e((b >> 16) & 0xFFu), e(b >> 24));
    }
}
// what a kernel of the count family is made of: the packed class's table in LDS, its per-read functor for a tile [glo, glo + gn) of the range
// [loc, loc + len), and how many words of a tile k_count_multi stages (the overlap forms carry loc and len too)
struct CountFamily {
    static constexpr int kStage = 16;
    template <int NT>
    static __device__ __forceinline__ void table(uint32_t *tab, const BsigKParams &P, int tid) { build_ctab<NT>(tab, P, tid); }
    static __device__ __forceinline__ CountOne make(const BsigKParams &P, int loc, int len, int glo, int gn, uint32_t &acc)
    {
        (void)loc; (void)len;
        return CountOne{P, glo, gn, acc};
    }
};
template <bool WITHIN>
struct OverlapFamily {
    static constexpr int kStage = 18;
    template <int NT>
    static __device__ __forceinline__ void table(uint32_t *tab, const BsigKParams &P, int tid) { build_otab<NT>(tab, P, tid); }
    static __device__ __forceinline__ OverlapOne<WITHIN> make(const BsigKParams &P, int loc, int len, int glo, int gn, uint32_t &acc)
    {
        return OverlapOne<WITHIN>{P, glo, gn, (int64_t)loc, (int64_t)loc + len - 1, acc};
    }
};

__global__ __launch_bounds__(128) void k_make_ptab(const BsigReadsDev R, const BsigKParams P, uint8_t *__restrict__ out)
{
    const int v = threadIdx.x;                              // four codes each: BSIG_PACK_CODES = 4 x 128
    uint32_t word = 0;
    if (4 * v < R.n_codes) {
        const uint4 f = reinterpret_cast<const uint4 *>(R.fmtab)[v];
        auto b = [&](uint32_t fm) { return (uint32_t)fm_rejected(P, fm) | ((fm >> 3) & 2u); };     // 0x10 >> 3
        word = b(f.x) | b(f.y) << 8 | b(f.z) << 16 | b(f.w) << 24;
    }
    reinterpret_cast<uint32_t *>(out)[v] = word;
}
static_assert(BSIG_PACK_CODES == 4 * 128, "k_make_ptab: four codes per thread of one 128-thread workgroup");

// The packed class's 16-bit column (bsig_types.h: p5h): the 5' end's low 15 bits and the strand, from a word
// (pos & 0x7FFF | (span - 1) << 15 | code << 23) and its code's pair; entries n .. cap - 1 are zero (16-B loads read them)
__global__ void k_make_p5h(const uint32_t *__restrict__ fm, const uint32_t *__restrict__ fmtab, int64_t n, int64_t cap,
                           uint16_t *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cap) return;
    uint32_t h = 0;
    if (i < n) {
        const uint32_t w = fm[i];
        const uint32_t rev = (fmtab[w >> 23] >> 4) & 1u;                      // 0x10: reverse strand (code < 512)
        const uint32_t p5 = (w & kPackPosMask) + (rev ? (w >> BSIG_PACK_POS_BITS) & 0xFFu : 0u);
        h = (p5 & kPackPosMask) | rev << 15;
    }
    out[i] = (uint16_t)h;
}

// The same column for span class 0 or 1 (bsig_types.h), from the class's pos and fm columns: span - 1 = fm >> span_shift
// (24 / 20), the strand is flag bit 0x10.  These classes also hold the reads whose pos lies outside their reference,
// which the bucket index files under the reference's first or last bucket: 15 bits of such a 5' end say nothing
// about where it is, so a class with one gets no column (*bad = 1).  A read is checked against the bucket the index
// has it in: the bucket idx[b] <= i < idx[b + 1] must be the one of its own position on the bucket's reference.
__global__ void k_make_short_p5h(const int32_t *__restrict__ pos, const uint32_t *__restrict__ fm, int span_shift, int64_t n, int64_t cap,
                                 const uint32_t *__restrict__ idx, uint64_t n_buckets, int kshift,
                                 const uint32_t *__restrict__ ref_unit0, const uint32_t *__restrict__ ref_units, int n_ref,
                                 uint16_t *__restrict__ out, int *__restrict__ bad)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cap) return;
    uint32_t h = 0;
    if (i < n) {
        uint64_t lo = 0, hi = n_buckets;                                      // idx[0] = 0 <= i < n = idx[n_buckets]
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            if ((int64_t)idx[mid] <= i) lo = mid; else hi = mid;
        }
        const uint64_t unit = (lo << kshift) >> BSIG_REF_UNIT_SHIFT;
        int r0 = 0, r1 = n_ref;                                               // last reference with ref_unit0 <= unit
        while (r1 - r0 > 1) {
            const int mid = (r0 + r1) >> 1;
            if ((uint64_t)ref_unit0[mid] <= unit) r0 = mid; else r1 = mid;
        }
        const int64_t p = pos[i], ref_bp = (int64_t)ref_units[r0] << BSIG_REF_UNIT_SHIFT;
        const bool inside = p >= 0 && p < ref_bp && ((((uint64_t)ref_unit0[r0] << BSIG_REF_UNIT_SHIFT) + (uint64_t)p) >> kshift) == lo;
        if (!inside) *bad = 1;
        const uint32_t w = fm[i];
        const uint32_t rev = (w >> 4) & 1u;
        const uint32_t p5 = (uint32_t)p + (rev ? w >> span_shift : 0u);
        h = (p5 & kPackPosMask) | rev << 15;
    }
    out[i] = (uint16_t)h;
}

// The packed class's window of a tile: the reads whose pos lies in the bucket-rounded window [rlo, rhi) of the
// reference, walked in chunks of kPackChunk bases (nearly always one): inside a chunk that starts at `base`,
// pos = base + ((word - base) & kPackPosMask).
struct PackedWin {
    int base;          // start of the first chunk (reference coordinate, a multiple of the bucket width)
    int n_chunks;      // 0: nothing to read
};

// Reads of class C that can touch the genomic interval [tlo, thi) lie in [j_lo, j_hi).
// pos in [tlo - ext - maxspan + 1, thi + ext), rounded outwards to index buckets.
// A resized plan (P.frag_len = L, covered_interval) has ext = L - 1, and that is enough: a forward read covers
// [pos, pos + L - 1], so one that reaches tlo has pos >= tlo - (L - 1) and one that starts before thi has pos < thi; a
// reverse read covers [end - L + 1, end], so one that starts before thi has pos <= end < thi + L - 1, and one that
// reaches tlo has end >= tlo, i.e. pos >= tlo - maxspan + 1, as a read that is not resized.  L below the span only trims.
__device__ __forceinline__ bool class_window(const BsigClassCols &C, const BsigWorkItem &w,
                                             int64_t tlo, int64_t thi, int ext,
                                             uint32_t &j_lo, uint32_t &j_hi)
{
    int64_t wlo = tlo - ext - C.maxspan + 1;
    int64_t whi = thi + ext;
    const int64_t ref_bp = (int64_t)(w.units_strand & BSIG_ITEM_UNITS_MASK) << BSIG_REF_UNIT_SHIFT;
    if (wlo < 0) wlo = 0;
    if (whi > ref_bp) whi = ref_bp;
    if (wlo >= whi) return false;
    const uint64_t g0 = (uint64_t)w.ref_unit0 << BSIG_REF_UNIT_SHIFT;
    const uint64_t b_lo = (g0 + (uint64_t)wlo) >> C.kshift;
    const uint64_t b_hi = (g0 + (uint64_t)whi - 1) >> C.kshift;
    j_lo = C.idx[b_lo];
    j_hi = C.idx[b_hi + 1];
    return j_lo < j_hi;
}

// genomic interval covered by a profile/coverage tile (cells [c0, c0+nc) in range orientation)
__device__ __forceinline__ void tile_interval(const BsigWorkItem &w, int binsize, bool neg_range,
                                              int64_t &tlo, int64_t &thi)
{
    const int64_t a = (int64_t)w.c0 * binsize;
    int64_t b = ((int64_t)w.c0 + w.nc) * binsize;
    if (b > w.len) b = w.len;
    if (neg_range) { tlo = (int64_t)w.loc + w.len - b; thi = (int64_t)w.loc + w.len - a; }
    else           { tlo = (int64_t)w.loc + a;         thi = (int64_t)w.loc + b; }
}

// Inclusive prefix sum over the 64 lanes of a wave in six DPP adds (no LDS traffic): a
// Hillis-Steele scan inside each row of 16 lanes (row_shr 1,2,4,8; lanes shifted in from outside
// the row read 0), then row 0 -> row 1 and row 2 -> row 3 (row_bcast:15), then lanes 0-31 ->
// lanes 32-63 (row_bcast:31).
__device__ __forceinline__ int wave_inclusive_scan(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true);     // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true);     // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true);     // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true);     // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);    // row_bcast:15 -> rows 1, 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);    // row_bcast:31 -> rows 2, 3
    return v;
}

// Pileup kernels take (items, n_tiles, out, windows) first: with -amdgpu-kernarg-preload-count=8
// (Makefile) those arrive in SGPRs, so the work-item load is issued with the first instruction
// instead of behind a kernarg fetch (config 2: 24.9 -> 24.6 us).  k_profile and k_profile_half take
// (items, n_tiles, img_vec, out, windows): items 2 dwords + n_tiles 1 + img_vec 1 + out 2 + windows 2 are exactly
// the eight preloaded ones -- img_vec fills the padding that stood between n_tiles and the 8-byte aligned `out`.
// Any further argument in front of `windows` pushes it out of the preload.
// Workgroups are dealt round-robin to the 8 XCDs (blocks b and b+8 share an L2), tiles are sorted
// by position: give every XCD one contiguous run of the tile list, so that neighbouring tiles,
// whose read windows overlap, meet in the same L2.  A bijection of [0, n); any mapping would be
// correct, this one is only faster (no assumption about WHICH XCD a block lands on).
__device__ __forceinline__ uint32_t tile_of_block(uint32_t b, uint32_t n)
{
    const uint32_t q = n >> 3, r = n & 7u, x = b & 7u, k = b >> 3;
    return x * q + (x < r ? x : r) + k;
}

template <int NT>
__device__ __forceinline__ void block_sync()
{
    // a 64-thread workgroup is one wave: LDS operations of a wave execute in order
    if (NT > kWave) __syncthreads();
    else __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

// Store nv values that sit at lds[sh .. sh+nv) to out[out_off .. out_off+nv): the LDS image is
// shifted by sh = out_off & 3 so that 16-B LDS vectors line up with 16-B aligned global addresses.
__device__ __forceinline__ void store_vec(int32_t *__restrict__ gbase, int v, int4 x, int sh, int nv)
{
    const int e0 = 4 * v;
    if (e0 >= sh && e0 + 4 <= sh + nv) {
        // the result is written once and never re-read by this launch: non-temporal stores keep
        // it from displacing the read columns in L2 (measured -6 % step time at config 2)
        typedef int v4i_t __attribute__((ext_vector_type(4)));
        v4i_t xv = {x.x, x.y, x.z, x.w};
        __builtin_nontemporal_store(xv, reinterpret_cast<v4i_t *>(gbase + e0));
    } else {
        const int lo = sh, hi = sh + nv;
        if (e0 + 0 >= lo && e0 + 0 < hi) gbase[e0 + 0] = x.x;
        if (e0 + 1 >= lo && e0 + 1 < hi) gbase[e0 + 1] = x.y;
        if (e0 + 2 >= lo && e0 + 2 < hi) gbase[e0 + 2] = x.z;
        if (e0 + 3 >= lo && e0 + 3 < hi) gbase[e0 + 3] = x.w;
    }
}

// a dword pair of a 16-bit tile image (two counters per LDS dword) as the four int32 cells it holds
__device__ __forceinline__ int4 widen16(uint2 d)
{
    return make_int4((int)(d.x & 0xFFFFu), (int)(d.x >> 16), (int)(d.y & 0xFFFFu), (int)(d.y >> 16));
}

// KB rows of NT interior vectors from row r0 on: all LDS reads issued before the first is consumed, then the 16-B
// non-temporal stores back to back, each under nothing but "this lane has a vector in this row"
template <int NT, int KB>
__device__ __forceinline__ void store_rows16(int4 *__restrict__ g4, const uint2 *__restrict__ l2, int tid, int r0, int n_int)
{
    typedef int v4i_t __attribute__((ext_vector_type(4)));
    uint2 d[KB];
#pragma unroll
    for (int k = 0; k < KB; ++k) {
        const int i = r0 + k * NT + tid;
        d[k] = l2[i < n_int ? i : n_int - 1];                        // (clamped, not masked: a read inside the image)
    }
#pragma unroll
    for (int k = 0; k < KB; ++k) {
        const int i = r0 + k * NT + tid;
        const int4 x = widen16(d[k]);
        const v4i_t xv = {x.x, x.y, x.z, x.w};
        if (i < n_int) __builtin_nontemporal_store(xv, reinterpret_cast<v4i_t *>(g4 + i));
    }
}

// The whole image of a tile whose cells are 16-bit counters (two per LDS dword), stored as store_vec would store its
// nvec vectors one by one -- but the interior vectors, those that lie in [sh, sh + nv) with all four values, go in
// batches (store_rows16): one LDS round trip for a batch instead of one per vector and lane.  sh and nv are uniform,
// so the interior is a run [v_lo, v_hi) with at most one edge vector on either side; those two keep store_vec's
// form, on two lanes.  The batch is sized to what is left of the run -- eight rows of NT vectors, four or two -- so
// that a 500- or 1,000-cell tile does not issue reads and store slots for rows it does not have.
template <int NT>
__device__ __forceinline__ void store_image16(int32_t *__restrict__ gbase, const uint2 *__restrict__ lds2, int tid, int sh, int nv)
{
    const int nvec = (sh + nv + 3) >> 2;
    const int v_lo = (sh + 3) >> 2, v_hi = (sh + nv) >> 2;          // interior: 4 v >= sh and 4 v + 4 <= sh + nv
    const int n_int = v_hi - v_lo;                                   // (<= 0: a tile inside one or two edge vectors)
    int4 *const g4 = reinterpret_cast<int4 *>(gbase) + v_lo;
    const uint2 *const l2 = lds2 + v_lo;
    for (int r0 = 0; r0 < n_int;) {                                  // (uniform)
        const int left = n_int - r0;
        if (left > 4 * NT)      { store_rows16<NT, 8>(g4, l2, tid, r0, n_int); r0 += 8 * NT; }
        else if (left > 2 * NT) { store_rows16<NT, 4>(g4, l2, tid, r0, n_int); r0 += 4 * NT; }
        else                    { store_rows16<NT, 2>(g4, l2, tid, r0, n_int); r0 += 2 * NT; }
    }
    // the edge vectors: vector 0 if the image starts inside it, the last one if the image ends inside it
    if (tid < 2 && nvec > 0) {
        const int v = tid ? nvec - 1 : 0;
        const bool edge = (v < v_lo || v >= v_hi) && (tid == 0 || nvec > 1);
        if (edge) store_vec(gbase, v, widen16(lds2[v]), sh, nv);
    }
}

// genomic interval a work item needs reads for
__device__ __forceinline__ void item_interval(const BsigWorkItem &w, const BsigKParams &P, int mode,
                                              int64_t &tlo, int64_t &thi)
{
    const bool neg_range = (w.units_strand & BSIG_ITEM_NEG) != 0u;
    if (mode == BSIG_MODE_COUNT) { tlo = (int64_t)w.loc + w.c0; thi = tlo + w.nc; }
    else tile_interval(w, P.binsize, neg_range, tlo, thi);        // (1 for per-base coverage)
}

// Index lookup for every (tile, class): windows[BSIG_MAX_CLASSES*t + c] = [j_lo, j_hi) of class c's reads
// that can touch tile t.  The device-side counterpart of bam_itr_queryi (src/bamsignals.cpp:267).
// Runs once per plan (bsig_plan_create probes the window sizes for heavy tiles); the pileup kernels look
// their windows up themselves (load_windows).
__global__ void k_resolve(const BsigReadsDev R, const BsigKParams P, int mode,
                          const BsigWorkItem *__restrict__ items, int64_t n_items,
                          uint2 *__restrict__ windows)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t t = g / BSIG_MAX_CLASSES;
    const int c = (int)(g - t * BSIG_MAX_CLASSES);
    if (t >= n_items) return;
    const BsigWorkItem w = items[t];
    int64_t tlo, thi;
    item_interval(w, P, mode, tlo, thi);
    uint32_t j_lo = 0, j_hi = 0;
    const BsigClassCols &C = R.cls[c];
    if (C.n == 0 || !class_window(C, w, tlo, thi, P.ext, j_lo, j_hi)) { j_lo = 0; j_hi = 0; }
    windows[g] = make_uint2(j_lo, j_hi);
}

// how many tiles hold more reads in their windows than `heavy_reads` (plan-time probe)
__global__ void k_count_heavy(const uint2 *__restrict__ windows, int64_t n_items, int64_t heavy_reads,
                              unsigned long long *__restrict__ count)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_items) return;
    int64_t total = 0;
#pragma unroll
    for (int c = 0; c < BSIG_MAX_CLASSES; ++c) {
        const uint2 w = windows[t * BSIG_MAX_CLASSES + c];
        total += (int64_t)w.y - w.x;
    }
    if (total > heavy_reads) atomicAdd(count, 1ull);
}

// class 1's word (flag (12 bits) | mapq << 12 | (span - 1) << 20, see read_class below) in the layout the
// filters read: flag | mapq << 16
__device__ __forceinline__ uint32_t fm_of_class1(uint32_t w) { return (w & 0xFFFu) | ((w >> 12) & 0xFFu) << 16; }

// four consecutive packed words (one lane's 16-B load) of a chunk that starts at `base`
// a per-read functor may bring its own treatment of four packed reads at once (`quad`): bamCount does
template <typename F, typename = void>
struct has_quad : std::false_type {};
template <typename F>
struct has_quad<F, std::void_t<decltype(&std::remove_reference_t<F>::quad)>> : std::true_type {};

template <typename Tab, typename F>
__device__ __forceinline__ void four_packed(const uint4 &w, const int4 &t, uint32_t j, uint32_t j_lo, uint32_t nj, int base,
                                            const Tab *__restrict__ ptab, F &&one, bool inner = false)
{
    if constexpr (has_quad<F>::value) {
        if constexpr (std::is_same_v<Tab, uint32_t>) one.quad(w, t, j - j_lo, nj, base, ptab, inner);      // (the count family)
        else one.quad(w, t, j - j_lo, nj, base, ptab);
        return;
    }
    // the four table bytes are requested before the first one is used
    const uint32_t b0 = ptab[w.x >> 23], b1 = ptab[w.y >> 23], b2 = ptab[w.z >> 23], b3 = ptab[w.w >> 23];
    const uint32_t dj = j - j_lo;
    auto dec = [&](uint32_t x, uint32_t b, int tl, bool valid) {
        const int pos = base + (int)((x - (uint32_t)base) & kPackPosMask);
        one(pos, pos + (int)((x >> BSIG_PACK_POS_BITS) & 0xFFu), (b & 2u) != 0u, (b & 1u) != 0u, tl, valid);
    };
    dec(w.x, b0, t.x, dj < nj);
    dec(w.y, b1, t.y, dj + 1u < nj);
    dec(w.z, b2, t.z, dj + 2u < nj);
    dec(w.w, b3, t.w, dj + 3u < nj);
}

// Stream the reads of all class windows of one tile through `one(pos, end, neg, rejected, tlen, valid)`
// (`rejected`: by the flag/mapq part of the filter).  Everything a typical tile needs is requested before
// anything is consumed, so the workgroup pays ONE memory round trip for its reads: the first kPre passes
// (kPre * 4 * NT reads) of the packed class, where nearly all reads live, and the first pass of classes 0
// and 1.  Longer windows and the two long-span classes continue in plain loops.
// (The packed class's later chunks -- windows wider than kPackChunk bases -- are walked by packed_later_chunks.)
// HALF (BsigKParams::packed_half, the functor has `oct`): the packed class comes from its 16-bit column p5h, eight
// reads per lane and 16-B load (passes of 8 * NT reads, no tlen column).  Under P.short_half classes 0 and 1 come from
// their 16-bit columns too: a window of up to NT reads as one half-word per lane (`half1`), requested where pos and
// fm are otherwise, a longer one eight reads per lane through `oct` with the class's own base (`short_base`).
template <int NT, int kPre = 2, bool HALF = false, typename Tab, typename F>
__device__ __forceinline__ void for_each_read(const BsigReadsDev &R, const BsigKParams &P,
                                              const uint2 (&win)[BSIG_MAX_CLASSES], int pbase,
                                              const Tab *__restrict__ ptab, int tid, F &&one)
{
    constexpr uint32_t kPer = HALF ? 8u : 4u;                        // packed reads per lane and 16-B load
    const bool use_tlen = !HALF && P.use_tlen;                       // (a plan with a template-length rule has no half form)
    uint4 w0[kPre];
    int4 t0[kPre];
    const BsigClassCols &CP = R.cls[BSIG_CLASS_PACKED];
    const uint32_t jbp = (win[BSIG_CLASS_PACKED].x & ~(kPer - 1u)) + kPer * tid;
#pragma unroll
    for (int k = 0; k < kPre; ++k) {
        const uint32_t j = jbp + kPer * NT * k;
        // (t0[k] is read under P.use_tlen only, which is when it is loaded: setting it to zero otherwise was four vector
        // instructions a pass in launches that are bound by exactly those)
        if (j < win[BSIG_CLASS_PACKED].y) {
            if constexpr (HALF) {
                w0[k] = *reinterpret_cast<const uint4 *>(CP.p5h + j);
            } else {
                w0[k] = *reinterpret_cast<const uint4 *>(CP.fm + j);
                if (P.use_tlen) t0[k] = *reinterpret_cast<const int4 *>(CP.tlen + j);
            }
        }
    }
    // The rare classes' windows are short -- the north star's tiles see some 20 reads of class 1 (the 5 % of reads
    // with a skipped region) -- and the launches are bound by their vector instructions, which a wave issues for all
    // its lanes or none: four reads per lane made such a window cost a whole pass of four `one`s (160 of a tile's 690
    // vector instructions).  A window of up to NT reads is taken ONE read per lane, requested here, ahead of the
    // packed class's work; a longer one is loaded where it is walked (the registers of a four-read prefetch held
    // across the packed class cost a wave per SIMD).
    const bool small0 = win[0].y - win[0].x <= (uint32_t)NT, small1 = win[1].y - win[1].x <= (uint32_t)NT;      // (uniform)
    int pa = 0, ta = 0, pb = 0, tb = 0;
    uint32_t fa = 0, fb = 0;
    const uint32_t jb0 = win[0].x + (uint32_t)tid, jb1 = win[1].x + (uint32_t)tid;
    // HALF under P.short_half (uniform): the lane's read is one half-word of the class's 16-bit column, which arrives in
    // fa / fb inside its dword.  The columns lie behind the packed class's (P.short_off), and the kernels read the flag
    // as short_win[1] != 0 (a bucket's log2 is never 0), a word they need anyway: with two more pointers and a flag of
    // its own in scalar registers k_profile_half<64, false, 2, 1, true> took 106 of them and a 33rd vector register
    // for the spills.
    auto short_now = [&]() {
        if constexpr (!HALF) return false;
        return P.short_win[1] != 0;
    };
    // ONE load per class serves both forms: the dword that holds the lane's half-word (the columns are 16-B aligned and
    // padded), or the lane's fm word -- a select of the column and a shift of the index, both uniform.  (A branch with
    // a load on either side made the pos + fm side wait for every load in flight before it issued its own: the two
    // sides share registers, and the wait counters are kept per block, not per path.)
    const bool sh_on = short_now();
    const uint32_t hs = sh_on ? 1u : 0u;
    const uint32_t *col0 = sh_on ? reinterpret_cast<const uint32_t *>(CP.p5h + P.short_off[0]) : R.cls[0].fm;
    const uint32_t *col1 = sh_on ? reinterpret_cast<const uint32_t *>(CP.p5h + P.short_off[1]) : R.cls[1].fm;
    if (small0 && jb0 < win[0].y) {
        fa = col0[jb0 >> hs];
        if (!sh_on) {
            pa = R.cls[0].pos[jb0];
            if (use_tlen) ta = R.cls[0].tlen[jb0];
        }
    }
    if (small1 && jb1 < win[1].y) {
        fb = col1[jb1 >> hs];
        if (!sh_on) {
            pb = R.cls[1].pos[jb1];
            if (use_tlen) tb = R.cls[1].tlen[jb1];
        }
    }
    // The 16-B aligned loads may start before j_lo (possibly on the previous reference) and end
    // after j_hi: only reads in [j_lo, j_hi) count -> `dj < nj` with unsigned wrap-around.
    if constexpr (HALF) {   // ---- packed class from p5h: one half-word per read ----------------------------
        (void)t0;
        const uint32_t j_lo = win[BSIG_CLASS_PACKED].x, j_hi = win[BSIG_CLASS_PACKED].y, nj = j_hi - j_lo;
#pragma unroll
        for (int k = 0; k < kPre; ++k) {
            const uint32_t j = jbp + 8u * NT * k;
            if (j < j_hi) one.oct(w0[k], j - j_lo, nj, pbase);
        }
        // deeper windows: two passes per trip, both requested before either is consumed
        for (uint32_t j = jbp + 8u * NT * kPre; j < j_hi; j += 16u * NT) {
            const uint32_t j2 = j + 8u * NT;
            const uint4 wa = *reinterpret_cast<const uint4 *>(CP.p5h + j);
            uint4 wb = make_uint4(0, 0, 0, 0);
            if (j2 < j_hi) wb = *reinterpret_cast<const uint4 *>(CP.p5h + j2);
            one.oct(wa, j - j_lo, nj, pbase);
            if (j2 < j_hi) one.oct(wb, j2 - j_lo, nj, pbase);
        }
    } else {   // ---- packed class (span <= 256, a frequent flag/mapq pair): one word per read -------------------
        const uint32_t j_lo = win[BSIG_CLASS_PACKED].x, j_hi = win[BSIG_CLASS_PACKED].y, nj = j_hi - j_lo;
        // a pass whose 4 * NT reads all belong to the window (uniform): nobody has to ask read by read
        const uint32_t jp0 = j_lo & ~3u;
        auto inner_pass = [&](uint32_t first) { return first >= j_lo && first + 4u * NT <= j_hi; };
#pragma unroll
        for (int k = 0; k < kPre; ++k) {
            const uint32_t j = jbp + 4u * NT * k;
            if (j < j_hi) four_packed(w0[k], t0[k], j, j_lo, nj, pbase, ptab, one, inner_pass(jp0 + 4u * NT * k));
        }
        // deeper windows: two passes per trip, both requested before either is consumed
        for (uint32_t j = jbp + 4u * NT * kPre, jf = jp0 + 4u * NT * kPre; j < j_hi; j += 8u * NT, jf += 8u * NT) {
            const uint32_t j2 = j + 4u * NT;
            const uint4 wa = *reinterpret_cast<const uint4 *>(CP.fm + j);
            int4 xa, xb;                                                   // (as t0: read under P.use_tlen only)
            uint4 wb = make_uint4(0, 0, 0, 0);
            if (P.use_tlen) xa = *reinterpret_cast<const int4 *>(CP.tlen + j);
            if (j2 < j_hi) {
                wb = *reinterpret_cast<const uint4 *>(CP.fm + j2);
                if (P.use_tlen) xb = *reinterpret_cast<const int4 *>(CP.tlen + j2);
            }
            four_packed(wa, xa, j, j_lo, nj, pbase, ptab, one, inner_pass(jf));
            if (j2 < j_hi) four_packed(wb, xb, j2, j_lo, nj, pbase, ptab, one, inner_pass(jf + 4u * NT));
        }
    }
    // ---- classes 0 and 1 from their 16-bit columns (P.short_half): the lane's half-word was requested above, the
    // class's base comes from the work item in scalar arithmetic; nothing but fa / fb and two words of the parameter
    // block was kept for them across the packed class's work
    if constexpr (HALF) {
        if (short_now()) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const uint32_t j_lo = win[c].x, j_hi = win[c].y, nj = j_hi - j_lo;
                if (!nj) continue;                                         // (uniform)
                const int base = one.short_base(c);
                if (c ? small1 : small0) {
                    one.half1(c ? fb >> ((jb1 & 1u) << 4) : fa >> ((jb0 & 1u) << 4), (c ? jb1 : jb0) < j_hi, base);
                } else
                for (uint32_t j = (j_lo & ~7u) + 8u * tid; j < j_hi; j += 8u * NT)
                    one.oct(*reinterpret_cast<const uint4 *>(CP.p5h + P.short_off[c] + j), j - j_lo, nj, base);
            }
        }
    }
    if (!short_now()) {
    {   // ---- class 0 (span <= 256, a rare pair): no end column, end = pos + (fm >> 24) ------------------
        const BsigClassCols &C = R.cls[0];
        const uint32_t j_lo = win[0].x, j_hi = win[0].y, nj = j_hi - j_lo;
        if (small0) {
            if (nj) one(pa, pa + (int)(fa >> 24), (fa & 0x10u) != 0u, fm_rejected(P, fa), ta, jb0 < j_hi);
        } else
        for (uint32_t j = (j_lo & ~3u) + 4u * tid; j < j_hi; j += 4u * NT) {
            const int4 p = *reinterpret_cast<const int4 *>(C.pos + j);
            const uint4 f = *reinterpret_cast<const uint4 *>(C.fm + j);
            int4 t = make_int4(0, 0, 0, 0);
            if (use_tlen) t = *reinterpret_cast<const int4 *>(C.tlen + j);
            const uint32_t dj = j - j_lo;
            one(p.x, p.x + (int)(f.x >> 24), (f.x & 0x10u) != 0u, fm_rejected(P, f.x), t.x, dj < nj);
            one(p.y, p.y + (int)(f.y >> 24), (f.y & 0x10u) != 0u, fm_rejected(P, f.y), t.y, dj + 1u < nj);
            one(p.z, p.z + (int)(f.z >> 24), (f.z & 0x10u) != 0u, fm_rejected(P, f.z), t.z, dj + 2u < nj);
            one(p.w, p.w + (int)(f.w >> 24), (f.w & 0x10u) != 0u, fm_rejected(P, f.w), t.w, dj + 3u < nj);
        }
    }
    {   // ---- class 1 (span <= 4096, 12-bit flags): no end column either, end = pos + (word >> 20) -----------
        const BsigClassCols &C = R.cls[1];
        const uint32_t j_lo = win[1].x, j_hi = win[1].y, nj = j_hi - j_lo;
        if (small1) {
            const uint32_t gx = fm_of_class1(fb);
            if (nj) one(pb, pb + (int)(fb >> 20), (gx & 0x10u) != 0u, fm_rejected(P, gx), tb, jb1 < j_hi);
        } else
        for (uint32_t j = (j_lo & ~3u) + 4u * tid; j < j_hi; j += 4u * NT) {
            const int4 p = *reinterpret_cast<const int4 *>(C.pos + j);
            const uint4 f = *reinterpret_cast<const uint4 *>(C.fm + j);
            int4 t = make_int4(0, 0, 0, 0);
            if (use_tlen) t = *reinterpret_cast<const int4 *>(C.tlen + j);
            const uint32_t dj = j - j_lo;
            const uint32_t gx = fm_of_class1(f.x), gy = fm_of_class1(f.y), gz = fm_of_class1(f.z), gw = fm_of_class1(f.w);
            one(p.x, p.x + (int)(f.x >> 20), (gx & 0x10u) != 0u, fm_rejected(P, gx), t.x, dj < nj);
            one(p.y, p.y + (int)(f.y >> 20), (gy & 0x10u) != 0u, fm_rejected(P, gy), t.y, dj + 1u < nj);
            one(p.z, p.z + (int)(f.z >> 20), (gz & 0x10u) != 0u, fm_rejected(P, gz), t.z, dj + 2u < nj);
            one(p.w, p.w + (int)(f.w >> 20), (gw & 0x10u) != 0u, fm_rejected(P, gw), t.w, dj + 3u < nj);
        }
    }
    }   // (!short_now())
#pragma unroll
    for (int c = 2; c < BSIG_SPAN_CLASSES; ++c) {   // ---- classes 2-3: pos, end, fm columns ---------
        const BsigClassCols &C = R.cls[c];
        const uint32_t j_lo = win[c].x, j_hi = win[c].y, nj = j_hi - j_lo;
        if (nj <= (uint32_t)NT) {                          // (one read per lane, as above)
            const uint32_t j = j_lo + (uint32_t)tid;
            if (nj) {
                int p = 0, e = 0, t = 0;
                uint32_t f = 0;
                if (j < j_hi) {
                    p = C.pos[j]; f = C.fm[j]; e = C.end[j];
                    if (use_tlen) t = C.tlen[j];
                }
                one(p, e, (f & 0x10u) != 0u, fm_rejected(P, f), t, j < j_hi);
            }
        } else
        for (uint32_t j = (j_lo & ~3u) + 4u * tid; j < j_hi; j += 4u * NT) {
            const int4 p = *reinterpret_cast<const int4 *>(C.pos + j);
            const uint4 f = *reinterpret_cast<const uint4 *>(C.fm + j);
            const int4 e = *reinterpret_cast<const int4 *>(C.end + j);
            int4 t = make_int4(0, 0, 0, 0);
            if (use_tlen) t = *reinterpret_cast<const int4 *>(C.tlen + j);
            const uint32_t dj = j - j_lo;
            one(p.x, e.x, (f.x & 0x10u) != 0u, fm_rejected(P, f.x), t.x, dj < nj);
            one(p.y, e.y, (f.y & 0x10u) != 0u, fm_rejected(P, f.y), t.y, dj + 1u < nj);
            one(p.z, e.z, (f.z & 0x10u) != 0u, fm_rejected(P, f.z), t.z, dj + 2u < nj);
            one(p.w, e.w, (f.w & 0x10u) != 0u, fm_rejected(P, f.w), t.w, dj + 3u < nj);
        }
    }
}

// the bucket-rounded window [rlo, rhi) of the packed class for the genomic interval [tlo, thi) of an item
__device__ __forceinline__ bool packed_window(const BsigClassCols &C, const BsigWorkItem &w, int64_t tlo, int64_t thi, int ext,
                                              int64_t &rlo, int64_t &rhi)
{
    int64_t wlo = tlo - ext - C.maxspan + 1, whi = thi + ext;
    const int64_t ref_bp = (int64_t)(w.units_strand & BSIG_ITEM_UNITS_MASK) << BSIG_REF_UNIT_SHIFT;
    if (wlo < 0) wlo = 0;
    if (whi > ref_bp) whi = ref_bp;
    rlo = (wlo >> C.kshift) << C.kshift;
    rhi = whi > 0 ? (((whi - 1) >> C.kshift) + 1) << C.kshift : 0;
    return C.n != 0 && wlo < whi;
}

// The packed class's chunks behind the first (a window wider than kPackChunk bases: a shift or a template
// length filter of tens of kilobases -- rare, so plain loops): every chunk is looked up in the index by
// itself and clipped to `clip` (the read range of a slice of a heavy tile; everything otherwise).
template <int NT, typename Tab, typename F>
__device__ __forceinline__ void packed_later_chunks(const BsigReadsDev &R, const BsigKParams &P, int mode, const BsigWorkItem &w,
                                                    int n_chunks, uint2 clip, const Tab *__restrict__ ptab, int tid, F &&one)
{
    const BsigClassCols &C = R.cls[BSIG_CLASS_PACKED];
    int64_t tlo, thi, rlo, rhi;
    item_interval(w, P, mode, tlo, thi);
    if (!packed_window(C, w, tlo, thi, P.ext, rlo, rhi)) return;
    const uint64_t g0 = (uint64_t)w.ref_unit0 << BSIG_REF_UNIT_SHIFT;
    for (int c = 1; c < n_chunks; ++c) {
        const int64_t a = rlo + (int64_t)c * kPackChunk;
        const int64_t b = a + kPackChunk < rhi ? a + kPackChunk : rhi;
        uint32_t j_lo = C.idx[(g0 + (uint64_t)a) >> C.kshift], j_hi = C.idx[(g0 + (uint64_t)b) >> C.kshift];
        j_lo = j_lo > clip.x ? j_lo : clip.x;
        j_hi = j_hi < clip.y ? j_hi : clip.y;
        if (j_lo >= j_hi) continue;
        const uint32_t nj = j_hi - j_lo;
        for (uint32_t j = (j_lo & ~3u) + 4u * tid; j < j_hi; j += 4u * NT) {
            const uint4 x = *reinterpret_cast<const uint4 *>(C.fm + j);
            int4 t = make_int4(0, 0, 0, 0);
            if (P.use_tlen) t = *reinterpret_cast<const int4 *>(C.tlen + j);
            four_packed(x, t, j, j_lo, nj, (int)a, ptab, one);
        }
    }
}

// The read windows of a tile, looked up here with the index loads of all classes issued back to back.
// `windows` (slices of heavy tiles): fixed read ranges instead -- for the span classes as they are, for the
// packed class as a clip of what the index says (the chunk's start is needed as well).
// P.resolved (large launches): the windows as k_resolve_tiles wrote them in front of this launch; a kernel
// instantiated with RES = true has nothing but that form in it (fewer registers).
template <bool RES = false>
__device__ __forceinline__ void load_windows(const BsigReadsDev &R, const BsigKParams &P, int mode,
                                             const BsigWorkItem &w, const BsigWorkItem *__restrict__ items,
                                             const uint2 *__restrict__ windows, uint2 (&win)[BSIG_MAX_CLASSES],
                                             uint32_t tile, PackedWin &pk, uint2 &clip)
{
    if (RES || P.resolved) {
        // the launch in front of this one looked the windows up (k_resolve_tiles): this load does not depend
        // on the work item's
        const BsigResolved r = reinterpret_cast<const BsigResolved *>(windows)[tile];
#pragma unroll
        for (int c = 0; c < BSIG_MAX_CLASSES; ++c) win[c] = make_uint2(r.win[2 * c], r.win[2 * c + 1]);
        pk.base = r.pbase;
        pk.n_chunks = r.pchunks;
        clip = make_uint2(0u, 0xFFFFFFFFu);
        return;
    }
    int64_t tlo, thi;
    item_interval(w, P, mode, tlo, thi);
    const uint32_t *alo[BSIG_MAX_CLASSES], *ahi[BSIG_MAX_CLASSES];
    bool live[BSIG_MAX_CLASSES];
    const int64_t ref_bp = (int64_t)(w.units_strand & BSIG_ITEM_UNITS_MASK) << BSIG_REF_UNIT_SHIFT;
    const uint64_t g0 = (uint64_t)w.ref_unit0 << BSIG_REF_UNIT_SHIFT;
    // dead classes read a harmless valid word instead of branching around the load
    const uint32_t *dummy = reinterpret_cast<const uint32_t *>(items);
#pragma unroll
    for (int c = 0; c < BSIG_SPAN_CLASSES; ++c) {
        const BsigClassCols &C = R.cls[c];
        int64_t wlo = tlo - P.ext - C.maxspan + 1, whi = thi + P.ext;
        if (wlo < 0) wlo = 0;
        if (whi > ref_bp) whi = ref_bp;
        live[c] = C.n != 0 && wlo < whi && !windows;
        alo[c] = live[c] ? C.idx + ((g0 + (uint64_t)wlo) >> C.kshift) : dummy;
        ahi[c] = live[c] ? C.idx + (((g0 + (uint64_t)whi - 1) >> C.kshift) + 1) : dummy;
    }
    {
        const BsigClassCols &C = R.cls[BSIG_CLASS_PACKED];
        int64_t rlo, rhi;
        const bool on = packed_window(C, w, tlo, thi, P.ext, rlo, rhi);
        live[BSIG_CLASS_PACKED] = on;
        const int64_t first_end = rlo + kPackChunk < rhi ? rlo + kPackChunk : rhi;
        alo[BSIG_CLASS_PACKED] = on ? C.idx + ((g0 + (uint64_t)rlo) >> C.kshift) : dummy;
        ahi[BSIG_CLASS_PACKED] = on ? C.idx + ((g0 + (uint64_t)first_end) >> C.kshift) : dummy;
        pk.base = (int)rlo;
        pk.n_chunks = on ? (int)((rhi - rlo + kPackChunk - 1) >> BSIG_PACK_POS_BITS) : 0;
    }
    uint32_t lo[BSIG_MAX_CLASSES], hi[BSIG_MAX_CLASSES];
#pragma unroll
    for (int c = 0; c < BSIG_MAX_CLASSES; ++c) { lo[c] = *alo[c]; hi[c] = *ahi[c]; }
#pragma unroll
    for (int c = 0; c < BSIG_MAX_CLASSES; ++c) win[c] = live[c] && lo[c] < hi[c] ? make_uint2(lo[c], hi[c]) : make_uint2(0u, 0u);
    clip = make_uint2(0u, 0xFFFFFFFFu);
    if (windows) {
        const uint2 *wp = windows + (size_t)BSIG_MAX_CLASSES * tile;
#pragma unroll
        for (int c = 0; c < BSIG_SPAN_CLASSES; ++c) win[c] = wp[c];
        clip = wp[BSIG_CLASS_PACKED];
        uint2 &q = win[BSIG_CLASS_PACKED];
        q.x = q.x > clip.x ? q.x : clip.x;
        q.y = q.y < clip.y ? q.y : clip.y;
        if (q.x >= q.y) q = make_uint2(0u, 0u);
    }
    // a heavy tile only zero-fills its cells here; its reads come through slice items afterwards
    if (w.units_strand & BSIG_ITEM_HEAVY) {
#pragma unroll
        for (int c = 0; c < BSIG_MAX_CLASSES; ++c) win[c] = make_uint2(0u, 0u);
        pk.n_chunks = 0;
    }
}

// The index lookups of a large launch as a launch of their own, one lane per tile: the pileup workgroups,
// which hold LDS and registers for their whole life, then start with their windows one load away.
__global__ void k_resolve_tiles(const BsigReadsDev R, const BsigKParams P, int mode,
                                const BsigWorkItem *__restrict__ items, uint32_t n_items,
                                BsigResolved *__restrict__ out)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_items) return;
    const BsigWorkItem w = items[t];
    uint2 win[BSIG_MAX_CLASSES], clip;
    PackedWin pk;
    load_windows(R, P, mode, w, items, nullptr, win, t, pk, clip);
    BsigResolved r;
#pragma unroll
    for (int c = 0; c < BSIG_MAX_CLASSES; ++c) { r.win[2 * c] = win[c].x; r.win[2 * c + 1] = win[c].y; }
    r.pbase = pk.base;
    r.pchunks = pk.n_chunks;
    out[t] = r;
}

// the accumulating form of store_vec: slices of a heavy tile add their (partial) image
__device__ __forceinline__ void add_vec(int32_t *__restrict__ gbase, int v, int4 x, int sh, int nv)
{
    const int e0 = 4 * v, lo = sh, hi = sh + nv;
    if (x.x && e0 + 0 >= lo && e0 + 0 < hi) atomicAdd(gbase + e0 + 0, x.x);
    if (x.y && e0 + 1 >= lo && e0 + 1 < hi) atomicAdd(gbase + e0 + 1, x.y);
    if (x.z && e0 + 2 >= lo && e0 + 2 < hi) atomicAdd(gbase + e0 + 2, x.z);
    if (x.w && e0 + 3 >= lo && e0 + 3 < hi) atomicAdd(gbase + e0 + 3, x.w);
}

// ------------------------------------------------------------------------------------------
// bamProfile: per-bin counts of 5' ends
// ------------------------------------------------------------------------------------------
// The tile image holds 16-bit counters, two per LDS dword: a tile that is not split into slices has
// at most 32,768 reads in its windows (kMaxTileReads; bsig_plan_create cuts anything above into
// slices of a quarter of that), so no counter can reach 65,536 and an add of 1 << 16 into the upper
// half never sees a carry from the lower one.  Half the LDS per workgroup: 24 instead of 18
// single-wave workgroups per CU (LDS is allocated in 1,280-byte granules on gfx950), which puts
// config 2's 10,000 tiles into two rounds of resident workgroups instead of two and a sparse third.
// HALF: the packed class from its 16-bit column (BsigKParams::packed_half) -- k_profile_half; the same body otherwise.
template <int NT, bool SS, int PRE, bool RES, bool HALF>
__device__ __forceinline__ void profile_tile(const BsigWorkItem *__restrict__ items, uint32_t n_tiles, int32_t *__restrict__ out,
                                             const uint2 *__restrict__ windows, const BsigReadsDev &R, const BsigKParams &P,
                                             uint32_t img_vec_launch)
{
    extern __shared__ __attribute__((aligned(16))) int32_t lds[];
    constexpr int S = SS ? 2 : 1;
    const int tid = threadIdx.x;
    BSIG_STAMP(0);
    const uint32_t tile = tile_of_block(blockIdx.x, n_tiles);
    const BsigWorkItem w = items[tile];
    uint2 win[BSIG_MAX_CLASSES], clip;
    PackedWin pk;
    load_windows<RES>(R, P, BSIG_MODE_PROFILE, w, items, windows, win, tile, pk, clip);
    int4 *lds4 = reinterpret_cast<int4 *>(lds);
    // clear the whole tile image: this needs nothing from the work item, so it overlaps its load -- and nothing from
    // the parameter block either, whose scalar loads return with the item's (scalar loads are waited for all at
    // once): the image's size in 16-B vectors is an argument of its own, the one that sized the launch's LDS, and
    // sits among the preloaded ones (= (P.tile_cells * S + 8 + 7) / 8)
    const int img_vec = (int)img_vec_launch;
    for (int v = tid; v < img_vec; v += NT) lds4[v] = make_int4(0, 0, 0, 0);
    // ... and so does the packed class's filter table, which lives behind the image
    uint8_t *ptab = reinterpret_cast<uint8_t *>(lds4 + img_vec);
    if (!HALF) build_ptab<NT>(ptab, R, P, tid);          // (the half form reads no table)
    const int nv = w.nc * S;
    const int sh = (int)(w.out_off & 3);
    const int nvec = (sh + nv + 3) >> 2;
    block_sync<NT>();
    BSIG_STAMP(1);

    const bool neg_range = (w.units_strand & BSIG_ITEM_NEG) != 0u;
    uint32_t *cnt = reinterpret_cast<uint32_t *>(lds);

    const ProfileOne<SS> one{P, cnt, w.loc, w.len, w.c0, w.nc, sh, neg_range};
    if (!BSIG_ABLATE(1)) {
        for_each_read<NT, PRE, HALF>(R, P, win, pk.base, ptab, tid, one);
        // (the half form's windows are one chunk: bsig_plan_create)
        if (!HALF && pk.n_chunks > 1) packed_later_chunks<NT>(R, P, BSIG_MODE_PROFILE, w, pk.n_chunks, clip, ptab, tid, one);
    }
    block_sync<NT>();
    BSIG_STAMP(2);

    int32_t *gbase = out + (w.out_off - sh);
    const uint2 *lds2 = reinterpret_cast<const uint2 *>(lds);
    if (P.accumulate) {
        for (int v = tid; v < nvec; v += NT) add_vec(gbase, v, widen16(lds2[v]), sh, nv);
    } else if (!BSIG_ABLATE(2)) {
        store_image16<NT>(gbase, lds2, tid, sh, nv);
    }
    BSIG_STAMP(3);
#ifdef BSIG_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    BSIG_STAMP(4);
    if (g_stamp_buf && threadIdx.x == 0) {
        unsigned xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        unsigned hwid;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
        g_stamp_buf[(size_t)blockIdx.x * 8 + 5] = ((unsigned long long)xcc << 32) | hwid;
    }
#endif
}
template <int NT, bool SS, int PRE, int WAVES, bool RES>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(WAVES, 8))) void k_profile(const BsigWorkItem *__restrict__ items, uint32_t n_tiles,
                                                uint32_t img_vec, int32_t *__restrict__ out,
                                                const uint2 *__restrict__ windows,
                                                const BsigReadsDev R, const BsigKParams P)
{
    profile_tile<NT, SS, PRE, RES, false>(items, n_tiles, out, windows, R, P, img_vec);
}
// k_profile reading the packed class's 16-bit column: a kernel of its own, so that the 4-byte form keeps its code
// (amdgpu_num_sgpr(102): the 100 scalar registers that eight waves per SIMD leave a wave, VCC included.  Left to itself
// the allocator takes up to 106 in the instantiations with looked-up windows, where the class-0/1 columns' offsets and
// window words are live beside the index lookups, and reports seven waves; the headline instantiations stay below
// the limit by themselves and spill nothing)
template <int NT, bool SS, int PRE, int WAVES, bool RES>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(WAVES, 8), amdgpu_num_sgpr(102))) void k_profile_half(const BsigWorkItem *__restrict__ items, uint32_t n_tiles,
                                                uint32_t img_vec, int32_t *__restrict__ out,
                                                const uint2 *__restrict__ windows,
                                                const BsigReadsDev R, const BsigKParams P)
{
    profile_tile<NT, SS, PRE, RES, true>(items, n_tiles, out, windows, R, P, img_vec);
}

// k_profile for T consecutive tiles per wave (large launches, windows from k_resolve_tiles): lane t fetches the work
// item and the windows of tile t of its group -- ONE round trip for the T tiles -- and parks them in LDS; the wave then
// works the tiles off one after the other through one image, which the store loop of a tile clears for the next.  From
// its second tile on a wave pays neither a workgroup launch, nor the item / windows trip, nor the filter table.
template <bool SS, int PRE, int T, bool HALF>
__device__ __forceinline__ void profile_multi_tiles(const BsigWorkItem *__restrict__ items, uint32_t n_tiles, int32_t *__restrict__ out,
                                                    const uint2 *__restrict__ windows, const BsigReadsDev &R, const BsigKParams &P)
{
    extern __shared__ __attribute__((aligned(16))) int32_t lds[];
    constexpr int S = SS ? 2 : 1;
    constexpr int kStage = 20;                               // dwords per tile: 8 of the item, 12 of its windows
    const int tid = threadIdx.x;
    const uint32_t n_groups = (n_tiles + T - 1) / T;
    const uint32_t first = tile_of_block(blockIdx.x, n_groups) * T;
    const uint32_t n_here = n_tiles - first < (uint32_t)T ? n_tiles - first : (uint32_t)T;      // uniform
    int4 *lds4 = reinterpret_cast<int4 *>(lds);
    const int img_vec = (P.tile_cells * S + 8 + 7) / 8;
    uint8_t *ptab = reinterpret_cast<uint8_t *>(lds4 + img_vec);
    uint32_t *stage = reinterpret_cast<uint32_t *>(ptab + BSIG_PACK_CODES);
    if ((uint32_t)tid < n_here) {
        const uint4 *ip = reinterpret_cast<const uint4 *>(items + first + tid);
        const uint4 *rp = reinterpret_cast<const uint4 *>(reinterpret_cast<const BsigResolved *>(windows) + first + tid);
        const uint4 a = ip[0], b = ip[1], c = rp[0], d = rp[1], e = rp[2];
        uint4 *sp = reinterpret_cast<uint4 *>(stage + kStage * tid);
        sp[0] = a; sp[1] = b; sp[2] = c; sp[3] = d; sp[4] = e;
    }
    for (int v = tid; v < img_vec; v += kWave) lds4[v] = make_int4(0, 0, 0, 0);
    if (!HALF) build_ptab<kWave>(ptab, R, P, tid);
    block_sync<kWave>();
    uint32_t *cnt = reinterpret_cast<uint32_t *>(lds);
    uint2 *lds2 = reinterpret_cast<uint2 *>(lds);
#pragma unroll 1
    for (uint32_t t = 0; t < n_here; ++t) {
        const uint32_t *sg = stage + kStage * t;
        auto sc = [&](int k) { return __builtin_amdgcn_readfirstlane((int)sg[k]); };
        BsigWorkItem w;
        w.loc = sc(0); w.len = sc(1); w.c0 = sc(2); w.nc = sc(3);
        w.out_off = (int64_t)(((uint64_t)(uint32_t)sc(5) << 32) | (uint32_t)sc(4));
        w.ref_unit0 = (uint32_t)sc(6); w.units_strand = (uint32_t)sc(7);
        uint2 win[BSIG_MAX_CLASSES];
#pragma unroll
        for (int c = 0; c < BSIG_MAX_CLASSES; ++c) win[c] = make_uint2((uint32_t)sc(8 + 2 * c), (uint32_t)sc(9 + 2 * c));
        const int pbase = sc(18), pchunks = sc(19);
        const int nv = w.nc * S;
        const int sh = (int)(w.out_off & 3);
        const int nvec = (sh + nv + 3) >> 2;
        const bool neg_range = (w.units_strand & BSIG_ITEM_NEG) != 0u;
        const ProfileOne<SS> one{P, cnt, w.loc, w.len, w.c0, w.nc, sh, neg_range};
        for_each_read<kWave, PRE, HALF>(R, P, win, pbase, ptab, tid, one);
        if (!HALF && pchunks > 1) packed_later_chunks<kWave>(R, P, BSIG_MODE_PROFILE, w, pchunks, make_uint2(0u, 0xFFFFFFFFu), ptab, tid, one);
        block_sync<kWave>();
        int32_t *gbase = out + (w.out_off - sh);
        for (int v = tid; v < nvec; v += kWave) {
            const uint2 d = lds2[v];
            lds2[v] = make_uint2(0u, 0u);                    // the image is the next tile's
            store_vec(gbase, v, make_int4((int)(d.x & 0xFFFFu), (int)(d.x >> 16), (int)(d.y & 0xFFFFu), (int)(d.y >> 16)), sh, nv);
        }
        block_sync<kWave>();
    }
}
template <bool SS, int PRE, int WAVES, int T>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(WAVES, 8))) void k_profile_multi(
    const BsigWorkItem *__restrict__ items, uint32_t n_tiles, int32_t *__restrict__ out, const uint2 *__restrict__ windows,
    const BsigReadsDev R, const BsigKParams P)
{
    profile_multi_tiles<SS, PRE, T, false>(items, n_tiles, out, windows, R, P);
}
template <bool SS, int PRE, int WAVES, int T>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(WAVES, 8))) void k_profile_multi_half(
    const BsigWorkItem *__restrict__ items, uint32_t n_tiles, int32_t *__restrict__ out, const uint2 *__restrict__ windows,
    const BsigReadsDev R, const BsigKParams P)
{
    profile_multi_tiles<SS, PRE, T, true>(items, n_tiles, out, windows, R, P);
}

// Wide bins (binsize >~ 8): a tile has few cells and thousands of reads, and the position-sorted
// reads of one wave instruction fall into one or two bins, so plain LDS atomics take turns on one or
// two addresses.  32-bit cells in LDS, a few replicas of the image (odd stride: the same cell of
// different replicas lies in different banks), summed at the end.
constexpr int kSmallCells = 256;     // at most this many values (cells * S) per tile
// Replicas of the image (lanes add into replica `tid & (r - 1)`, the replicas are summed at the end): FEW, and chosen by
// the TILE's own values.  Rounds 2-4 kept up to 32 (8 KiB) so that no two lanes of a wave would meet on a cell; clearing
// and summing r x values dwords per tile and the LDS they take cost more than lanes taking turns (100,000 x 2 kb ranges,
// 1e8 reads, one box; 32 / 4 / 2 / 1 replicas: binsize 50 with strands (80 values) 0.167 / 0.117 / 0.114 / 0.107 ms,
// binsize 16 (125 values) 0.174 / 0.116 / 0.113 / 0.107): four replicas for images of up to 32 values, two up to 64, one
// beyond.  With a handful of cells they matter most -- one replica instead of four: binsize 2000 with strands (two
// values) 0.107 -> 0.172 ms, binsize 500 (four values) 0.105 -> 0.24 -- and until late in round 5 the choice went by the
// PLAN's tile_cells, which is never below 64: a 2-kb range in bins of 200 bases (10 cells, 20 values with strands) ran
// with one replica.  By the tile's values: binsize 200 with strands 0.1235 -> 0.110 ms, binsize 500 0.139 -> 0.105.
// (Spreading the lanes over the window instead -- a lane takes consecutive vectors, so that an instruction's reads come
// from all over the tile -- does the same for 20 values and nothing once the replicas are right: not kept.)
__host__ __device__ inline int small_replicas(int stride)
{
    return stride <= 32 ? 4 : stride <= 64 ? 2 : 1;
}
// dwords of the largest image (replicas x odd stride) a tile of at most `stride_max` values can ask for
__host__ __device__ inline int small_image_dwords(int stride_max)
{
    int most = stride_max * small_replicas(stride_max);          // (strides are odd: 31 and 63 are the last of their kind)
    if (stride_max > 31) most = most > 31 * small_replicas(31) ? most : 31 * small_replicas(31);
    if (stride_max > 63) most = most > 63 * small_replicas(63) ? most : 63 * small_replicas(63);
    return most;
}
template <int NT, bool SS, bool RES>
__global__ __launch_bounds__(NT) void k_profile_small(const BsigWorkItem *__restrict__ items, uint32_t n_tiles,
                                                      int32_t *__restrict__ out,
                                                      const uint2 *__restrict__ windows,
                                                      const BsigReadsDev R, const BsigKParams P)
{
    extern __shared__ __attribute__((aligned(16))) int32_t lds[];
    constexpr int S = SS ? 2 : 1;
    const int tid = threadIdx.x;
    const uint32_t tile = tile_of_block(blockIdx.x, n_tiles);
    const BsigWorkItem w = items[tile];
    uint2 win[BSIG_MAX_CLASSES], clip;
    PackedWin pk;
    load_windows<RES>(R, P, BSIG_MODE_PROFILE, w, items, windows, win, tile, pk, clip);
    // the replicas go by THIS tile's values (a plan's tile_cells is at least 64 cells); the launch reserves the image of
    // the worst tile a plan of this tile_cells can hold
    const int nv = w.nc * S;
    const int stride = nv | 1;                                 // odd: replicas shift by one bank
    const int n_rep = small_replicas(stride);
    for (int v = tid; v < n_rep * stride; v += NT) lds[v] = 0;
    uint8_t *ptab = reinterpret_cast<uint8_t *>(lds + ((small_image_dwords((P.tile_cells * S) | 1) + 3) & ~3));
    build_ptab<NT>(ptab, R, P, tid);
    block_sync<NT>();
    const bool neg_range = (w.units_strand & BSIG_ITEM_NEG) != 0u;
    int32_t *mine = lds + (tid & (n_rep - 1)) * stride;

    const SmallOne<SS> one{P, mine, w.loc, w.len, w.c0, w.nc, neg_range};
#ifndef BSIG_SMALL_PRE
#define BSIG_SMALL_PRE 4
#endif
    for_each_read<NT, BSIG_SMALL_PRE>(R, P, win, pk.base, ptab, tid, one);
    if (pk.n_chunks > 1) packed_later_chunks<NT>(R, P, BSIG_MODE_PROFILE, w, pk.n_chunks, clip, ptab, tid, one);
    block_sync<NT>();

    for (int v = tid; v < nv; v += NT) {
        int acc = 0;
        for (int r = 0; r < n_rep; ++r) acc += lds[r * stride + v];
        if (!P.accumulate) out[w.out_off + v] = acc;
        else if (acc) atomicAdd(out + w.out_off + v, acc);
    }
}

// ------------------------------------------------------------------------------------------
// bamCount: one (or two, strand-specific) counters per range
// ------------------------------------------------------------------------------------------
// (the body of k_count and of k_overlap: Fam is CountFamily or OverlapFamily<WITHIN>)
template <int NT, typename Fam>
__device__ __forceinline__ void count_tile(const BsigWorkItem *__restrict__ items, uint32_t n_tiles,
                                           int32_t *__restrict__ out,
                                           const uint2 *__restrict__ windows,
                                           const BsigReadsDev &R, const BsigKParams &P)
{
    __shared__ int32_t wsum[2 * (NT / kWave)];
    __shared__ __attribute__((aligned(16))) uint32_t ptab[BSIG_PACK_CODES];      // (the count family's table: Fam::table)
    const int tid = threadIdx.x;
    const uint32_t tile = tile_of_block(blockIdx.x, n_tiles);
    const BsigWorkItem w = items[tile];
    uint2 win[BSIG_MAX_CLASSES], clip;
    PackedWin pk;
    load_windows(R, P, BSIG_MODE_COUNT, w, items, windows, win, tile, pk, clip);
    Fam::template table<NT>(ptab, P, tid);
    block_sync<NT>();
    const bool neg_range = (w.units_strand & BSIG_ITEM_NEG) != 0u;
    const int glo = w.loc + w.c0;           // sub-interval of the range, genomic coordinates
    const int gn = w.nc;
    // Counting is all this launch does per read, and the launch is bound by its vector instructions (PMC, config 3's
    // tiling: 95e6 VALU instructions x 4 cycles over 1,024 SIMDs = the whole 155 us): no branch per read -- a read
    // that is no read, rejected or outside adds 0 -- and ONE packed counter (all reads in its low half, reverse-strand
    // ones in its high half) that becomes sense and antisense once, behind the loop.
    uint32_t acc = 0;
    const auto one = Fam::make(P, w.loc, w.len, glo, gn, acc);
    for_each_read<NT>(R, P, win, pk.base, ptab, tid, one);
    if (pk.n_chunks > 1) packed_later_chunks<NT>(R, P, BSIG_MODE_COUNT, w, pk.n_chunks, clip, ptab, tid, one);
    const int c_all = (int)(acc & 0xFFFFu), c_neg = (int)(acc >> 16);
    int c_anti = neg_range ? c_all - c_neg : c_neg, c_sense = c_all - c_anti;

    // wave reduction, then across the waves of the workgroup
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) {
        c_sense += __shfl_down(c_sense, d);
        c_anti += __shfl_down(c_anti, d);
    }
    if (NT > kWave) {
        if ((tid & (kWave - 1)) == 0) { wsum[2 * (tid / kWave)] = c_sense; wsum[2 * (tid / kWave) + 1] = c_anti; }
        __syncthreads();
        if (tid == 0) {
            c_sense = 0; c_anti = 0;
            for (int k = 0; k < NT / kWave; ++k) { c_sense += wsum[2 * k]; c_anti += wsum[2 * k + 1]; }
        }
    }
    if (tid == 0) {
        const bool atomic = (w.units_strand & BSIG_ITEM_ATOMIC) != 0u;
        int32_t *o = out + w.out_off;
        if (P.ss) {
            if (atomic) { if (c_sense) atomicAdd(o, c_sense); if (c_anti) atomicAdd(o + 1, c_anti); }
            else        { o[0] = c_sense; o[1] = c_anti; }
        } else {
            if (atomic) { if (c_sense + c_anti) atomicAdd(o, c_sense + c_anti); }
            else        { o[0] = c_sense + c_anti; }
        }
    }
}
template <int NT>
__global__ __launch_bounds__(NT) void k_count(const BsigWorkItem *__restrict__ items, uint32_t n_tiles,
                                              int32_t *__restrict__ out,
                                              const uint2 *__restrict__ windows,
                                              const BsigReadsDev R, const BsigKParams P)
{
    count_tile<NT, CountFamily>(items, n_tiles, out, windows, R, P);
}
// bamOverlaps: k_count's body with OverlapOne<WITHIN> per read (a tile counts the reads anchored in it)
template <int NT, bool WITHIN>
__global__ __launch_bounds__(NT) void k_overlap(const BsigWorkItem *__restrict__ items, uint32_t n_tiles,
                                                int32_t *__restrict__ out,
                                                const uint2 *__restrict__ windows,
                                                const BsigReadsDev R, const BsigKParams P)
{
    count_tile<NT, OverlapFamily<WITHIN>>(items, n_tiles, out, windows, R, P);
}

// bamCount, several consecutive tiles per wave.  A count tile moves one dword out and has no LDS image,
// so nothing but the dependent chain item -> index -> reads fills a wave's lifetime.  Here lane t of
// the wave fetches the work item of tile t of its group and looks up that tile's windows (T chains
// side by side instead of one behind the other); the tiles are then streamed one after the other
// with the windows broadcast from their lane, and lane t stores tile t's counters at the end.
// (the body of k_count_multi and of k_overlap_multi)
template <int T, int PRE, typename Fam>
__device__ __forceinline__ void count_multi_tiles(const BsigWorkItem *__restrict__ items, uint32_t n_tiles,
                                                  int32_t *__restrict__ out,
                                                  const uint2 *__restrict__ windows,
                                                  const BsigReadsDev &R, const BsigKParams &P)
{
    // per tile: 5 windows, first base, bases, flags, packed base and chunks (the overlap forms: the range's loc and len)
    __shared__ uint32_t stage[T][Fam::kStage];
    __shared__ __attribute__((aligned(16))) uint32_t ptab[BSIG_PACK_CODES];      // (the count family's table: Fam::table)
    const int lane = threadIdx.x;
    const uint32_t n_groups = (n_tiles + T - 1) / T;
    const uint32_t first = tile_of_block(blockIdx.x, n_groups) * T;
    const uint32_t n_here = n_tiles - first < (uint32_t)T ? n_tiles - first : (uint32_t)T;      // uniform
    const bool have = (uint32_t)lane < n_here;
    int64_t out_off = 0;
    bool atomic = false;
    if (have) {
        const BsigWorkItem w = items[first + lane];
        uint2 win[BSIG_MAX_CLASSES], clip;
        PackedWin pk;
        load_windows(R, P, BSIG_MODE_COUNT, w, items, windows, win, first + lane, pk, clip);
#pragma unroll
        for (int c = 0; c < BSIG_MAX_CLASSES; ++c) { stage[lane][2 * c] = win[c].x; stage[lane][2 * c + 1] = win[c].y; }
        stage[lane][10] = (uint32_t)(w.loc + w.c0);
        stage[lane][11] = (uint32_t)w.nc;
        stage[lane][12] = w.units_strand;
        stage[lane][13] = (uint32_t)pk.base;
        stage[lane][14] = (uint32_t)pk.n_chunks;
        if constexpr (Fam::kStage > 16) { stage[lane][16] = (uint32_t)w.loc; stage[lane][17] = (uint32_t)w.len; }
        out_off = w.out_off;
        atomic = (w.units_strand & BSIG_ITEM_ATOMIC) != 0u;
    }
    Fam::template table<kWave>(ptab, P, lane);
    block_sync<kWave>();
    int my_sense = 0, my_anti = 0;
#pragma unroll 1
    for (int t = 0; t < (int)n_here; ++t) {
        uint2 wn[BSIG_MAX_CLASSES];
#pragma unroll
        for (int c = 0; c < BSIG_MAX_CLASSES; ++c)
            wn[c] = make_uint2((uint32_t)__builtin_amdgcn_readfirstlane((int)stage[t][2 * c]),
                               (uint32_t)__builtin_amdgcn_readfirstlane((int)stage[t][2 * c + 1]));
        const int glo = __builtin_amdgcn_readfirstlane((int)stage[t][10]);
        const int gn = __builtin_amdgcn_readfirstlane((int)stage[t][11]);
        const bool neg_range = ((uint32_t)__builtin_amdgcn_readfirstlane((int)stage[t][12]) & BSIG_ITEM_NEG) != 0u;
        const int pbase = __builtin_amdgcn_readfirstlane((int)stage[t][13]);
        const int pchunks = __builtin_amdgcn_readfirstlane((int)stage[t][14]);
        int loc = 0, len = 0;
        if constexpr (Fam::kStage > 16) {
            loc = __builtin_amdgcn_readfirstlane((int)stage[t][16]);
            len = __builtin_amdgcn_readfirstlane((int)stage[t][17]);
        }
        uint32_t acc = 0;                          // (see k_count: nothing branches per read)
        const auto one = Fam::make(P, loc, len, glo, gn, acc);
        for_each_read<kWave, PRE>(R, P, wn, pbase, ptab, lane, one);
        if (pchunks > 1) {
            const BsigWorkItem w2 = items[first + t];
            packed_later_chunks<kWave>(R, P, BSIG_MODE_COUNT, w2, pchunks, make_uint2(0u, 0xFFFFFFFFu), ptab, lane, one);
        }
        // (the wave's sum stays packed: a tile that is not sliced has at most 32,768 reads in its windows)
        // (six DPP adds and a v_readlane; the butterfly of __shfl_xor was six trips through LDS and their addresses)
        const uint32_t sum = (uint32_t)__builtin_amdgcn_readlane(wave_inclusive_scan((int)acc), kWave - 1);
        const int c_all = (int)(sum & 0xFFFFu), c_neg = (int)(sum >> 16);
        const int c_anti = neg_range ? c_all - c_neg : c_neg, c_sense = c_all - c_anti;
        if (lane == t) { my_sense = c_sense; my_anti = c_anti; }
    }
    if (have) {
        int32_t *o = out + out_off;
        if (P.ss) {
            if (atomic) { if (my_sense) atomicAdd(o, my_sense); if (my_anti) atomicAdd(o + 1, my_anti); }
            else        { o[0] = my_sense; o[1] = my_anti; }
        } else {
            if (atomic) { if (my_sense + my_anti) atomicAdd(o, my_sense + my_anti); }
            else        { o[0] = my_sense + my_anti; }
        }
    }
}
template <int T, int PRE>
__global__ __launch_bounds__(kWave) void k_count_multi(const BsigWorkItem *__restrict__ items, uint32_t n_tiles,
                                                       int32_t *__restrict__ out,
                                                       const uint2 *__restrict__ windows,
                                                       const BsigReadsDev R, const BsigKParams P)
{
    count_multi_tiles<T, PRE, CountFamily>(items, n_tiles, out, windows, R, P);
}
template <int T, int PRE, bool WITHIN>
__global__ __launch_bounds__(kWave) void k_overlap_multi(const BsigWorkItem *__restrict__ items, uint32_t n_tiles,
                                                         int32_t *__restrict__ out,
                                                         const uint2 *__restrict__ windows,
                                                         const BsigReadsDev R, const BsigKParams P)
{
    count_multi_tiles<T, PRE, OverlapFamily<WITHIN>>(items, n_tiles, out, windows, R, P);
}

// ------------------------------------------------------------------------------------------
// bamCoverage: +1/-1 difference array in LDS, workgroup prefix scan, coalesced store
// ------------------------------------------------------------------------------------------
// The difference array holds SIGNED 16-bit cells, two per LDS dword, as k_profile's image does with
// unsigned ones: the dword is kept equal to hi * 65536 + lo (mod 2^32) by plain integer adds of
// +-1 and +-65536 (a borrow out of the low half is part of that sum, not an error), and is taken
// apart at the end as lo = sign-extended low half, hi = sign-extended high half of (word + 0x8000).
// A tile that is not cut into slices has at most 32,767 reads in its windows (bsig_plan_create's
// ceiling for coverage), so every cell stays inside [-32767, 32767].  4 KiB instead of 8 KiB of
// LDS per 2,048-cell tile: 24 instead of 18 single-wave workgroups per CU.
template <int NT, int PRE, bool RES, bool FRAG = false>
__global__ __launch_bounds__(NT) void k_coverage(const BsigWorkItem *__restrict__ items, uint32_t n_tiles,
                                                 int32_t *__restrict__ out,
                                                 const uint2 *__restrict__ windows,
                                                 const BsigReadsDev R, const BsigKParams P)
{
    extern __shared__ __attribute__((aligned(16))) int32_t lds[];
    const int img_vec = (P.tile_cells + 8 + 7) / 8;          // 16-B vectors of the image (8 cells each)
    // per-wave scan totals live behind the tile image, inside the dynamic region, so that the
    // image itself starts at the 16-B aligned LDS base
    int32_t *wtot = lds + 4 * img_vec;
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const uint32_t tile = tile_of_block(blockIdx.x, n_tiles);
    const BsigWorkItem w = items[tile];
    uint2 win[BSIG_MAX_CLASSES], clip;
    PackedWin pk;
    load_windows<RES>(R, P, BSIG_MODE_COVERAGE, w, items, windows, win, tile, pk, clip);
    int4 *lds4 = reinterpret_cast<int4 *>(lds);
    for (int v = tid; v < img_vec; v += NT) lds4[v] = make_int4(0, 0, 0, 0);
    // the packed class's filter table: behind the image and the scan totals (16-B aligned)
    uint8_t *ptab = reinterpret_cast<uint8_t *>(lds4 + img_vec + (NT / kWave + 3) / 4);
    build_ptab<NT>(ptab, R, P, tid);
    const int nv = w.nc;
    const int sh = (int)(w.out_off & 3);
    const int nvec = (sh + nv + 3) >> 2;
    block_sync<NT>();

    const bool neg_range = (w.units_strand & BSIG_ITEM_NEG) != 0u;
    const int rend1 = w.loc + w.len - 1;     // last base of the range

    const CoverOneT<FRAG> one{P, lds, w.loc, w.c0, w.nc, sh, neg_range, rend1};
    for_each_read<NT, PRE>(R, P, win, pk.base, ptab, tid, one);
    if (pk.n_chunks > 1) packed_later_chunks<NT>(R, P, BSIG_MODE_COVERAGE, w, pk.n_chunks, clip, ptab, tid, one);
    block_sync<NT>();

    // cumsum (:464-470): each lane owns 4 consecutive cells (two packed dwords), wave scan of the
    // lane totals, carry across waves and across passes
    int32_t *gbase = out + (w.out_off - sh);
    const uint2 *lds2 = reinterpret_cast<const uint2 *>(lds);
    auto lo16 = [](uint32_t d) { return (int)(int16_t)(uint16_t)d; };
    auto hi16 = [](uint32_t d) { return (int)(int16_t)(uint16_t)((d + 0x8000u) >> 16); };
    int carry = 0;
    for (int base = 0; base < nvec; base += NT) {
        const int v = base + tid;
        const uint2 d = v < nvec ? lds2[v] : make_uint2(0u, 0u);
        int4 x = make_int4(lo16(d.x), hi16(d.x), lo16(d.y), hi16(d.y));
        x.y += x.x; x.z += x.y; x.w += x.z;
        const int tot = x.w;
        const int incl = wave_inclusive_scan(tot);
        int pre = carry;
        int all = __builtin_amdgcn_readlane(incl, kWave - 1);
        if (NT > kWave) {
            if (lane == kWave - 1) wtot[tid / kWave] = incl;
            __syncthreads();
            all = 0;
            for (int k = 0; k < NT / kWave; ++k) {
                const int t = wtot[k];
                if (k < tid / kWave) pre += t;
                all += t;
            }
            __syncthreads();
        }
        const int add = pre + incl - tot;
        x.x += add; x.y += add; x.z += add; x.w += add;
        if (v < nvec) {
            if (P.accumulate) add_vec(gbase, v, x, sh, nv);
            else store_vec(gbase, v, x, sh, nv);
        }
        carry += all;
    }
}

// ------------------------------------------------------------------------------------------
// bamCoverage in bins of b bases and/or split by strand: the per-base coverage summed over each bin
// ------------------------------------------------------------------------------------------
// A read covers the bases [ra, rb] of the tile (range orientation, clipped to the tile), i.e. a tail h of
// its first bin ja, every base of the bins between, and a head t of its last bin jb.  The tile keeps ONE
// int32 difference image D whose prefix sum is the bin value: D[ja] += h, D[ja+1] += b - h, D[jb] += t - b,
// D[jb+1] -= t (two adds if ja == jb, three if jb == ja + 1): at most four LDS atomics a read, whatever its
// span.  Each read adds at most b to a cell in magnitude, and a tile that is not cut into slices has at most
// 32,767 reads in its windows, so with b <= 65,536 neither a cell of D nor any prefix of it can leave int32.
// With SS the image holds cell 2*bin + antisense -- the result's own order -- and the two rows are scanned
// apart.
// The reads of a pass are consecutive in position, so with wide bins most lanes of a wave add to the same one or two
// cells, and LDS atomics to one address execute one after the other: the image is kept in P.cov_reps copies (lane l
// adds to copy l % reps; copies lie an odd number of 16-B vectors apart, so one cell's copies sit in different banks),
// summed when the scan reads them.
template <bool SS, bool FRAG = false>
struct CoverBinsOne {
    const BsigKParams &P;
    int32_t *img;
    int loc, c0, nc, sh;
    bool neg_range;
    int rend1;                              // last base of the range
    int lo, hi;                             // the tile's bases in range orientation, [lo, hi]
    __device__ __forceinline__ int bin_of(int x) const
    {
        return P.binsize == 1 ? x : (int)(__umulhi((uint32_t)x, P.div_magic) >> P.div_shift);
    }
    __device__ __forceinline__ void operator()(int p, int e, bool neg, bool rej, int tl, bool valid) const
    {
        if (!valid || rej || tlen_rejected(P, tl)) return;            // ref: src/bamsignals.cpp:394-399
        int start, end;
        covered_interval<FRAG>(P, p, e, neg, tl, start, end);        // (a fragment keeps this read's strand)
        int ra = neg_range ? rend1 - end : start - loc;
        int rb = neg_range ? rend1 - start : end - loc;
        ra = ra > lo ? ra : lo;
        rb = rb < hi ? rb : hi;
        if (ra > rb) return;
        const int b = P.binsize;
        const int ga = bin_of(ra), gb = bin_of(rb);
        const int ja = ga - c0, jb = gb - c0;
        constexpr int S = SS ? 2 : 1;
        const int k = sh + (SS && neg != neg_range ? 1 : 0);         // antisense: the read's strand is not the range's
        if (ja == jb) {
            const int n = rb - ra + 1;
            atomicAdd(&img[k + S * ja], n);
            if (ja + 1 < nc) atomicAdd(&img[k + S * (ja + 1)], -n);
            return;
        }
        const int h = b - (ra - ga * b), t = rb - gb * b + 1;
        atomicAdd(&img[k + S * ja], h);
        atomicAdd(&img[k + S * (ja + 1)], jb == ja + 1 ? t - h : b - h);
        if (jb > ja + 1) atomicAdd(&img[k + S * jb], t - b);
        if (jb + 1 < nc) atomicAdd(&img[k + S * (jb + 1)], -t);
    }
};

// add_vec for binned coverage: every addend is >= 0, so an add that takes a cell past INT32_MAX is told by the
// value it returns; it raises the plan's flag, and the host fails the call instead of returning a wrapped value
__device__ __forceinline__ void add_vec_checked(int32_t *__restrict__ gbase, int v, int4 x, int sh, int nv,
                                                int32_t *__restrict__ overflow)
{
    const int e0 = 4 * v, lo = sh, hi = sh + nv;
    bool over = false;
    auto one = [&](int e, int a) {
        if (a && e >= lo && e < hi) over |= (int64_t)atomicAdd(gbase + e, a) + a > (int64_t)INT32_MAX;
    };
    one(e0 + 0, x.x);
    one(e0 + 1, x.y);
    one(e0 + 2, x.z);
    one(e0 + 3, x.w);
    if (over) atomicOr(overflow, 1);
}

// 16-B vectors of one copy of a k_coverage_bins image of `cells` cells (+ the shift), odd; and the copies a launch
// keeps: as many as fit 8 KiB, at most 16 (env BAMSIGNALS_COVERAGE_REPLICAS: 1, 2, 4, 8 or 16 instead)
__host__ __device__ __forceinline__ int cov_bins_vec(int cells) { return ((cells + 7) / 4) | 1; }
static int cov_bins_reps(int cells)
{
    static const int forced = getenv("BAMSIGNALS_COVERAGE_REPLICAS") ? atoi(getenv("BAMSIGNALS_COVERAGE_REPLICAS")) : 0;
    if (forced == 1 || forced == 2 || forced == 4 || forced == 8 || forced == 16) return forced;
    int r = 1;
    while (r < 16 && 2 * r * cov_bins_vec(cells) * 16 <= 8192) r *= 2;
    return r;
}

template <int NT, int PRE, bool RES, bool SS, bool FRAG = false>
__global__ __launch_bounds__(NT) void k_coverage_bins(const BsigWorkItem *__restrict__ items, uint32_t n_tiles,
                                                      int32_t *__restrict__ out,
                                                      const uint2 *__restrict__ windows,
                                                      const BsigReadsDev R, const BsigKParams P)
{
    extern __shared__ __attribute__((aligned(16))) int32_t lds[];
    constexpr int S = SS ? 2 : 1;
    constexpr int NW = NT / kWave;
    const int img_vec = cov_bins_vec(P.tile_cells * S);        // 16-B vectors of one copy (4 cells each, shift included)
    const int reps = P.cov_reps;
    int32_t *wtot = lds + 4 * img_vec * reps;                  // per-wave scan totals (S of them), behind the copies
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const uint32_t tile = tile_of_block(blockIdx.x, n_tiles);
    const BsigWorkItem w = items[tile];
    uint2 win[BSIG_MAX_CLASSES], clip;
    PackedWin pk;
    load_windows<RES>(R, P, BSIG_MODE_COVERAGE, w, items, windows, win, tile, pk, clip);
    int4 *lds4 = reinterpret_cast<int4 *>(lds);
    for (int v = tid; v < img_vec * reps; v += NT) lds4[v] = make_int4(0, 0, 0, 0);
    uint8_t *ptab = reinterpret_cast<uint8_t *>(lds4 + img_vec * reps + (S * NW + 3) / 4);
    build_ptab<NT>(ptab, R, P, tid);
    const int nv = w.nc * S;
    const int sh = (int)(w.out_off & 3);                       // (even with SS: a range's cells come in pairs)
    const int nvec = (sh + nv + 3) >> 2;
    block_sync<NT>();

    const bool neg_range = (w.units_strand & BSIG_ITEM_NEG) != 0u;
    const int lo = w.c0 * P.binsize;
    const int64_t tile_end = ((int64_t)w.c0 + w.nc) * P.binsize;
    const int hi = (int)(tile_end < w.len ? tile_end : (int64_t)w.len) - 1;
    const CoverBinsOne<SS, FRAG> one{P, lds + 4 * img_vec * (lane & (reps - 1)), w.loc, w.c0, w.nc, sh, neg_range, w.loc + w.len - 1, lo, hi};
    for_each_read<NT, PRE>(R, P, win, pk.base, ptab, tid, one);
    if (pk.n_chunks > 1) packed_later_chunks<NT>(R, P, BSIG_MODE_COVERAGE, w, pk.n_chunks, clip, ptab, tid, one);
    block_sync<NT>();

    // prefix sum of D (per row with SS): each lane owns 4 consecutive cells, wave scan of the lane totals, carry
    // across waves and across passes
    int32_t *gbase = out + (w.out_off - sh);
    int carry0 = 0, carry1 = 0;
    for (int base = 0; base < nvec; base += NT) {
        const int v = base + tid;
        int4 x = make_int4(0, 0, 0, 0);
        if (v < nvec)
            for (int r = 0; r < reps; ++r) {
                const int4 y = lds4[r * img_vec + v];
                x.x += y.x; x.y += y.y; x.z += y.z; x.w += y.w;
            }
        int tot0, tot1 = 0;
        if (SS) { x.z += x.x; x.w += x.y; tot0 = x.z; tot1 = x.w; }      // cells (bin, row): (j,0) (j,1) (j+1,0) (j+1,1)
        else    { x.y += x.x; x.z += x.y; x.w += x.z; tot0 = x.w; }
        const int incl0 = wave_inclusive_scan(tot0);
        const int incl1 = SS ? wave_inclusive_scan(tot1) : 0;
        int pre0 = carry0, pre1 = carry1;
        int all0 = __builtin_amdgcn_readlane(incl0, kWave - 1);
        int all1 = SS ? __builtin_amdgcn_readlane(incl1, kWave - 1) : 0;
        if (NW > 1) {
            if (lane == kWave - 1) { wtot[S * (tid / kWave)] = incl0; if (SS) wtot[S * (tid / kWave) + 1] = incl1; }
            __syncthreads();
            all0 = 0; all1 = 0;
            for (int k = 0; k < NW; ++k) {
                const int t0 = wtot[S * k], t1 = SS ? wtot[S * k + 1] : 0;
                if (k < tid / kWave) { pre0 += t0; pre1 += t1; }
                all0 += t0; all1 += t1;
            }
            __syncthreads();
        }
        const int add0 = pre0 + incl0 - tot0, add1 = pre1 + incl1 - tot1;
        if (SS) { x.x += add0; x.z += add0; x.y += add1; x.w += add1; }
        else    { x.x += add0; x.y += add0; x.z += add0; x.w += add0; }
        if (v < nvec) {
            if (P.accumulate) add_vec_checked(gbase, v, x, sh, nv, P.overflow);
            else store_vec(gbase, v, x, sh, nv);
        }
        carry0 += all0; carry1 += all1;
    }
}

// ------------------------------------------------------------------------------------------
// Sums over ranges of one width (bsig_plan_create_sum): the metaprofile of alignSignals + rowMeans
// ------------------------------------------------------------------------------------------
// The plan tiles every range per base (bins come last: binning is linear) and orders its tiles by c0, so that all
// tiles of one c0 -- one tile position in range orientation, the same nc for every range -- are consecutive.  A
// workgroup owns a run of tiles of ONE c0 (bsig_plan_create_sum never lets a run cross a c0 or hold more than 65,536
// tiles).  Its NW waves take the run's tiles in turn, each wave on its own tile and 16-bit image with the read bodies
// of the per-range kernels (ProfileOne, CoverOne; CoverBinsOne at binsize 1 with strands), so that NW item -> windows
// -> reads chains are in flight per workgroup.  A finished image is folded into the workgroup's 32-bit accumulator
// with LDS atomics and cleared for the wave's next tile; at the end the accumulator is stored once, as the run's slab
// (plain 16-B stores).  Exact: an unsliced tile adds at most 32,768 to a cell (a coverage difference at most 32,767 in
// magnitude) and a slice of a heavy tile less, so 65,536 tiles stay below 2^32 unsigned (2^31 signed).
enum { kSumProfile = 0, kSumCover = 1, kSumCoverSS = 2 };

template <int NW, int KIND, bool SS, bool HALF, bool RES, bool FRAG = false>
__global__ __launch_bounds__(NW * kWave) void k_sum_tiles(const BsigWorkItem *__restrict__ items, const uint2 *__restrict__ runs,
                                                          int32_t *__restrict__ slab, const uint2 *__restrict__ windows,
                                                          const BsigReadsDev R, const BsigKParams P)
{
    extern __shared__ __attribute__((aligned(16))) int32_t lds[];
    constexpr int NT = NW * kWave;
    constexpr int S = SS ? 2 : 1;
    constexpr int mode = KIND == kSumProfile ? BSIG_MODE_PROFILE : BSIG_MODE_COVERAGE;
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wv = __builtin_amdgcn_readfirstlane(tid / kWave);
    const int vals = P.tile_cells * S;
    const int acc_v = (vals + 3) / 4;                                        // 16-B vectors of the accumulator
    const int img_v = KIND == kSumCoverSS ? (vals + 3) / 4 : (vals + 7) / 8; // ... of one wave's image
    int4 *lds4 = reinterpret_cast<int4 *>(lds);
    uint32_t *acc = reinterpret_cast<uint32_t *>(lds);
    int32_t *img = lds + 4 * (acc_v + img_v * wv);
    uint8_t *ptab = reinterpret_cast<uint8_t *>(lds4 + acc_v + img_v * NW);
    for (int v = tid; v < acc_v + img_v * NW; v += NT) lds4[v] = make_int4(0, 0, 0, 0);
    if (!HALF) build_ptab<NT>(ptab, R, P, tid);
    const uint2 run = runs[blockIdx.x];
    __syncthreads();

#pragma unroll 1
    for (uint32_t t = run.x + (uint32_t)wv; t < run.y; t += NW) {
        const BsigWorkItem w = items[t];
        uint2 win[BSIG_MAX_CLASSES], clip;
        PackedWin pk;
        load_windows<RES>(R, P, mode, w, items, windows, win, t, pk, clip);
        const bool neg_range = (w.units_strand & BSIG_ITEM_NEG) != 0u;
        if constexpr (KIND == kSumProfile) {
            const ProfileOne<SS> one{P, reinterpret_cast<uint32_t *>(img), w.loc, w.len, w.c0, w.nc, 0, neg_range};
            for_each_read<kWave, 2, HALF>(R, P, win, pk.base, ptab, lane, one);
            if (!HALF && pk.n_chunks > 1) packed_later_chunks<kWave>(R, P, mode, w, pk.n_chunks, clip, ptab, lane, one);
        } else if constexpr (KIND == kSumCover) {
            const CoverOneT<FRAG> one{P, img, w.loc, w.c0, w.nc, 0, neg_range, w.loc + w.len - 1};
            for_each_read<kWave, 2>(R, P, win, pk.base, ptab, lane, one);
            if (pk.n_chunks > 1) packed_later_chunks<kWave>(R, P, mode, w, pk.n_chunks, clip, ptab, lane, one);
        } else {
            const int hi = (w.c0 + w.nc < w.len ? w.c0 + w.nc : w.len) - 1;
            const CoverBinsOne<true, FRAG> one{P, img, w.loc, w.c0, w.nc, 0, neg_range, w.loc + w.len - 1, w.c0, hi};
            for_each_read<kWave, 2>(R, P, win, pk.base, ptab, lane, one);
            if (pk.n_chunks > 1) packed_later_chunks<kWave>(R, P, mode, w, pk.n_chunks, clip, ptab, lane, one);
        }
        block_sync<kWave>();
        // fold the image into the accumulator and clear it for this wave's next tile
        const int nv = w.nc * S;
        if constexpr (KIND == kSumCoverSS) {
            for (int v = lane; v < nv; v += kWave) {
                const int x = img[v];
                img[v] = 0;
                if (x) atomicAdd(&acc[v], (uint32_t)x);
            }
        } else {
            uint32_t *im = reinterpret_cast<uint32_t *>(img);
            for (int v = lane; 2 * v < nv; v += kWave) {
                const uint32_t d = im[v];
                im[v] = 0u;
                // profile: two unsigned 16-bit counters; coverage: two signed 16-bit differences (see k_coverage)
                const uint32_t a = KIND == kSumProfile ? d & 0xFFFFu : (uint32_t)(int)(int16_t)(uint16_t)d;
                const uint32_t b = KIND == kSumProfile ? d >> 16 : (uint32_t)(int)(int16_t)(uint16_t)((d + 0x8000u) >> 16);
                if (a) atomicAdd(&acc[2 * v], a);
                if (b) atomicAdd(&acc[2 * v + 1], b);
            }
        }
        block_sync<kWave>();
    }
    __syncthreads();
    int4 *dst = reinterpret_cast<int4 *>(slab + (size_t)blockIdx.x * (size_t)(4 * acc_v));
    for (int v = tid; v < acc_v; v += NT) dst[v] = lds4[v];
}

// The slabs of the runs of one c0, a chunk of at most kSumChunkSlots of them at a time, added into the per-base sums
// (int64, cell x * S + s of the range-oriented width; zeroed in front): one thread per four cells, unsigned slabs for
// profiles, signed ones for coverage differences
template <bool SIGNED>
__global__ __launch_bounds__(256) void k_sum_reduce(const int32_t *__restrict__ slab, int32_t slab_vals, const BsigSumChunk *__restrict__ chunks,
                                                    unsigned long long *__restrict__ base)
{
    const BsigSumChunk c = chunks[blockIdx.y];
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (4 * v >= c.nvals) return;
    int64_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    for (uint32_t k = c.slot_lo; k < c.slot_hi; ++k) {
        const int4 x = reinterpret_cast<const int4 *>(slab + (size_t)k * (size_t)slab_vals)[v];
        if (SIGNED) { s0 += x.x; s1 += x.y; s2 += x.z; s3 += x.w; }
        else { s0 += (uint32_t)x.x; s1 += (uint32_t)x.y; s2 += (uint32_t)x.z; s3 += (uint32_t)x.w; }
    }
    unsigned long long *o = base + c.cell0 + 4 * v;
    const int left = c.nvals - 4 * v;
    if (s0) atomicAdd(o + 0, (unsigned long long)s0);
    if (left > 1 && s1) atomicAdd(o + 1, (unsigned long long)s1);
    if (left > 2 && s2) atomicAdd(o + 2, (unsigned long long)s2);
    if (left > 3 && s3) atomicAdd(o + 3, (unsigned long long)s3);
}

// Coverage: the summed difference images become summed coverage by a prefix sum that RESTARTS at every tile boundary
// c0 (each tile's image is self-contained: a read that crosses a boundary starts in both tiles).  One workgroup per
// (tile position, row): each thread scans up to 32 consecutive cells, the workgroup scans the thread totals.
__global__ __launch_bounds__(256) void k_sum_scan(long long *__restrict__ base, int32_t width, int32_t tile_cells, int32_t S)
{
    __shared__ long long tot[256];
    const int q = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
    const int c0 = q * tile_cells;
    const int nc = width - c0 < tile_cells ? width - c0 : tile_cells;
    const int per = (nc + 255) / 256;
    const int a = tid * per, b = a + per < nc ? a + per : nc;
    long long run = 0;
    for (int i = a; i < b; ++i) run += base[(size_t)(c0 + i) * S + s];
    tot[tid] = run;
    __syncthreads();
    for (int d = 1; d < 256; d *= 2) {           // inclusive Hillis-Steele scan of the thread totals
        const long long y = tid >= d ? tot[tid - d] : 0;
        __syncthreads();
        tot[tid] += y;
        __syncthreads();
    }
    long long acc = tot[tid] - run;
    for (int i = a; i < b; ++i) {
        long long *p = base + (size_t)(c0 + i) * S + s;
        acc += *p;
        *p = acc;
    }
}

// Bins in range orientation: out[2 * bin + s] (out[bin] without strands) = the per-base sums of the bin's bases
// [bin * binsize, min((bin + 1) * binsize, width)); one thread per cell for narrow bins, one wave per cell for wide ones
template <bool WAVE>
__global__ __launch_bounds__(256) void k_sum_bins(const long long *__restrict__ base, int32_t width, int32_t binsize, int32_t S,
                                                  int64_t n_out, long long *__restrict__ out)
{
    const int64_t g = WAVE ? (int64_t)blockIdx.x * 4 + threadIdx.x / kWave : (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= n_out) return;
    const int64_t j = g / S, s = g - j * S;
    const int64_t x0 = j * binsize, x1 = x0 + binsize < width ? x0 + binsize : width;
    long long sum = 0;
    if (WAVE) {
        for (int64_t x = x0 + (threadIdx.x & (kWave - 1)); x < x1; x += kWave) sum += base[x * S + s];
        for (int m = kWave / 2; m >= 1; m /= 2) sum += __shfl_xor(sum, m);
        if ((threadIdx.x & (kWave - 1)) == 0) out[g] = sum;
    } else {
        for (int64_t x = x0; x < x1; ++x) sum += base[x * S + s];
        out[g] = sum;
    }
}

// ------------------------------------------------------------------------------------------
// Strand cross-correlation over ranges (bsig_plan_create_xcorr)
// ------------------------------------------------------------------------------------------
// A tile is a BODY of consecutive cells of one range (w.out_off of them: an xcorr tile writes no per-range cells) and an
// antisense HALO behind it, w.nc = body + halo cells in all, halo = min(max_lag, cells left in the range).  A workgroup
// owns a run of tiles.  Per tile it piles the 5' ends up per strand into an LDS image with the per-range read bodies
// (ProfileOne<true>: dword x holds sense[x] in its low half and antisense[x] in its high half), compacts the body's
// non-zero sense cells into a list, and then every lane takes lags d = tid, tid + NT, ... : for each it walks the list
// and adds S[x] * A[x + d] -- consecutive lanes read consecutive LDS dwords, the list entry is a broadcast -- two lags
// at a time, so that one list read serves two multiply-adds.  Cells of the image behind the tile's nc are zero (the
// read bodies mask on nc), so a lag that runs past the range's end adds nothing and needs no test.
// Exactness.  16-bit image: an unsliced tile has at most 32,768 reads in its windows and each counts in one cell, so
// sum(S) + sum(A) <= 2^15 and a lag's sum over the tile is at most sum(S) * max(A) <= 2^28: a 32-bit register per lag
// and tile, flushed after every tile into the lag's 64-bit LDS accumulator (owned by one lane: plain adds).  WIDE
// (tiles with more reads, which the plan lists apart): 32-bit cells, read by read, 64-bit registers.  The plan proves
// that no 64-bit sum reaches 2^63.  At the end of its run a workgroup adds its non-zero partial sums to the result with
// one 64-bit atomic per lag, and its four moment sums with one per wave.

// the read-by-read body of a WIDE tile: 32-bit cells, 2 * cell + antisense (shift 0, bins of one base)
struct XcorrWideOne {
    const BsigKParams &P;
    uint32_t *cnt;
    int loc, len, c0, nc;
    bool neg_range;
    __device__ __forceinline__ void operator()(int p, int e, bool neg, bool rej, int tl, bool valid) const
    {
        if (!valid || rej || tlen_rejected(P, tl)) return;
        int rel = (neg ? e : p) - loc;
        if ((unsigned)rel >= (unsigned)len) return;
        int anti = neg ? 1 : 0;
        if (neg_range) { rel = len - rel - 1; anti ^= 1; }
        const int lc = rel - c0;
        if ((unsigned)lc < (unsigned)nc) atomicAdd(&cnt[2 * lc + anti], 1u);
    }
};

// ... and its sibling for a plan with a shift (the capped 5' ends): the 5' end moves by P.shift in the read's own direction,
// as ProfileOne moves it
struct ShiftedWideOne {
    const BsigKParams &P;
    uint32_t *cnt;
    int loc, len, c0, nc;
    bool neg_range;
    __device__ __forceinline__ void operator()(int p, int e, bool neg, bool rej, int tl, bool valid) const
    {
        if (!valid || rej || tlen_rejected(P, tl)) return;
        int rel = (neg ? e - P.shift : p + P.shift) - loc;
        if ((unsigned)rel >= (unsigned)len) return;
        int anti = neg ? 1 : 0;
        if (neg_range) { rel = len - rel - 1; anti ^= 1; }
        const int lc = rel - c0;
        if ((unsigned)lc < (unsigned)nc) atomicAdd(&cnt[2 * lc + anti], 1u);
    }
};
// a consumer of walk_tile_cells that declares kShifted takes ShiftedWideOne for its wide tiles
template <typename C, typename = void>
struct wants_shift : std::false_type {};
template <typename C>
struct wants_shift<C, std::void_t<decltype(C::kShifted)>> : std::true_type {};

// LDS of one k_xcorr_tiles workgroup, in dwords: image | list | 64-bit lag accumulators | counter (+ pad) | filter table
struct XcorrLds {
    int img, list, acc, misc, ptab, total;
};
__host__ __device__ inline XcorrLds xcorr_lds(bool wide, int tile_cells, int body, int max_lag)
{
    XcorrLds L;
    L.img = 0;
    L.list = ((wide ? 2 : 1) * tile_cells + 8 + 3) & ~3;
    L.acc = (L.list + body + 3) & ~3;
    L.misc = L.acc + 2 * (max_lag + 1);
    L.ptab = L.misc + 4;
    L.total = L.ptab + BSIG_PACK_CODES / 4;
    return L;
}

template <int NT, bool HALF, bool WIDE>
__global__ __launch_bounds__(NT) void k_xcorr_tiles(const BsigWorkItem *__restrict__ items, const uint2 *__restrict__ runs,
                                                    unsigned long long *__restrict__ out, const uint2 *__restrict__ windows,
                                                    const BsigReadsDev R, const BsigKParams P, int body, int max_lag,
                                                    unsigned long long n_cells)
{
    extern __shared__ __attribute__((aligned(16))) int32_t lds[];
    typedef typename std::conditional<WIDE, unsigned long long, uint32_t>::type acc_t;
    const int tid = threadIdx.x;
    const XcorrLds L = xcorr_lds(WIDE, P.tile_cells, body, max_lag);
    uint32_t *img = reinterpret_cast<uint32_t *>(lds) + L.img;
    uint32_t *list = reinterpret_cast<uint32_t *>(lds) + L.list;
    unsigned long long *lag = reinterpret_cast<unsigned long long *>(lds + L.acc);
    uint32_t *nnz = reinterpret_cast<uint32_t *>(lds) + L.misc;
    uint8_t *ptab = reinterpret_cast<uint8_t *>(lds + L.ptab);
    for (int v = tid; v < L.misc + 4; v += NT) lds[v] = 0;
    if (!HALF) build_ptab<NT>(ptab, R, P, tid);
    const uint2 run = runs[blockIdx.x];
    unsigned long long m_s = 0, m_a = 0, m_ss = 0, m_aa = 0;
    __syncthreads();

#pragma unroll 1
    for (uint32_t t = run.x; t < run.y; ++t) {
        const BsigWorkItem w = items[t];
        uint2 win[BSIG_MAX_CLASSES], clip;
        PackedWin pk;
        load_windows<false>(R, P, BSIG_MODE_PROFILE, w, items, windows, win, t, pk, clip);
        const bool neg_range = (w.units_strand & BSIG_ITEM_NEG) != 0u;
        if constexpr (WIDE) {
            const XcorrWideOne one{P, img, w.loc, w.len, w.c0, w.nc, neg_range};
            for_each_read<NT, 2, false>(R, P, win, pk.base, ptab, tid, one);
            if (pk.n_chunks > 1) packed_later_chunks<NT>(R, P, BSIG_MODE_PROFILE, w, pk.n_chunks, clip, ptab, tid, one);
        } else {
            const ProfileOne<true> one{P, img, w.loc, w.len, w.c0, w.nc, 0, neg_range};
            for_each_read<NT, 2, HALF>(R, P, win, pk.base, ptab, tid, one);
            if (!HALF && pk.n_chunks > 1) packed_later_chunks<NT>(R, P, BSIG_MODE_PROFILE, w, pk.n_chunks, clip, ptab, tid, one);
        }
        __syncthreads();
        // the body's moments, and its non-zero sense cells into the list (in any order: a sum)
        const int nb = (int)w.out_off;
        for (int x = tid; x < nb; x += NT) {
            const uint32_t s = WIDE ? img[2 * x] : img[x] & 0xFFFFu, a = WIDE ? img[2 * x + 1] : img[x] >> 16;
            m_s += s; m_a += a;
            m_ss += (unsigned long long)s * s; m_aa += (unsigned long long)a * a;
            if (s) list[atomicAdd(nnz, 1u)] = WIDE ? (uint32_t)x : (uint32_t)x | s << 16;
        }
        __syncthreads();
        const int n = (int)*nnz;
        if (2 * (max_lag + 1) <= NT) {
            // fewer lags than half the lanes: G groups of PW >= max_lag + 1 lanes share the list, entry i to group
            // i mod G, and meet in the lag's accumulator with an LDS atomic
            int PW = 1;
            while (PW < max_lag + 1) PW <<= 1;
            const int d = tid & (PW - 1), G = NT / PW;
            if (d <= max_lag) {
                acc_t a0 = 0;
                for (int i = tid / PW; i < n; i += G) {
                    const uint32_t e = list[i];
                    if constexpr (WIDE) a0 += (unsigned long long)img[2 * e] * img[2 * (e + d) + 1];
                    else a0 += (e >> 16) * (img[(e & 0xFFFFu) + d] >> 16);
                }
                if (a0) atomicAdd(&lag[d], (unsigned long long)a0);
            }
        } else
        // lags tid + k NT, two per pass; a second lag beyond max_lag walks the first one's cells and is dropped
        for (int d0 = tid; d0 <= max_lag; d0 += 2 * NT) {
            const int d1 = d0 + NT;
            const bool two = d1 <= max_lag;
            const int e1 = two ? d1 : d0;
            acc_t a0 = 0, a1 = 0;
            for (int i = 0; i < n; ++i) {
                const uint32_t e = list[i];
                if constexpr (WIDE) {
                    const unsigned long long s = img[2 * e];
                    a0 += s * img[2 * (e + d0) + 1];
                    a1 += s * img[2 * (e + e1) + 1];
                } else {
                    const uint32_t x = e & 0xFFFFu, s = e >> 16;
                    a0 += s * (img[x + d0] >> 16);
                    a1 += s * (img[x + e1] >> 16);
                }
            }
            lag[d0] += a0;
            if (two) lag[d1] += a1;
        }
        __syncthreads();
        // the image and the list's counter, cleared for the run's next tile
        for (int v = tid; v < (WIDE ? 2 : 1) * w.nc; v += NT) img[v] = 0u;
        if (tid == 0) *nnz = 0u;
        __syncthreads();
    }
    for (int d = tid; d <= max_lag; d += NT)
        if (lag[d]) atomicAdd(out + d, lag[d]);
    for (int m = kWave / 2; m >= 1; m /= 2) {
        m_s += __shfl_xor(m_s, m); m_a += __shfl_xor(m_a, m);
        m_ss += __shfl_xor(m_ss, m); m_aa += __shfl_xor(m_aa, m);
    }
    if ((tid & (kWave - 1)) == 0) {
        unsigned long long *mo = out + max_lag + 1;          // moments: [cells (the plan's count), sum S, sum A, sum S^2, sum A^2]
        if (blockIdx.x == 0 && tid == 0 && n_cells) atomicAdd(mo, n_cells);
        if (m_s) atomicAdd(mo + 1, m_s);
        if (m_a) atomicAdd(mo + 2, m_a);
        if (m_ss) atomicAdd(mo + 3, m_ss);
        if (m_aa) atomicAdd(mo + 4, m_aa);
    }
}

// ------------------------------------------------------------------------------------------
// Fragment-length histogram over ranges (bsig_plan_create_frag)
// ------------------------------------------------------------------------------------------
// A tile is a sub-interval [loc + c0, loc + c0 + nc) of a range, as a count tile is; it has no image.  A workgroup owns a
// run of tiles and keeps ONE histogram of n_rows 32-bit counters in LDS for all of them: a read that is the first of a
// proper pair (the plan's flag masks), whose |tlen| = a lies in the filter and whose position -- its 5' end, moved by
// a / 2 under the midpoint rule -- lies in the tile adds 1 to row a / lenbin.  At the end of its run the workgroup adds
// its non-zero rows to the int64 result with one 64-bit atomic each.
// Exactness.  Every read in a tile's windows adds at most 1, and the plan cuts the runs so that the reads in a run's
// windows stay below 2^32 (runtime.hip: frag_setup): no LDS counter wraps.  a < 2^31 is divided by lenbin with the
// round-up multiplier of host_util.h (magic_u31), full width: a reaches 2^30, so no 24-bit multiply touches it or the
// midpoint offset.
// Contention.  All increments of a run land on n_rows LDS cells, and real lengths crowd onto a few hundred of them; a
// pile of duplicates puts every lane of a wave on ONE cell, which the LDS serves one lane per cycle.  MERGE: the lanes
// that hold the same row as the wave's first accepted lane are counted with a ballot and added by that lane alone; the
// other rows take their own atomics.  A pile then costs one LDS cycle instead of 64; a wave of all-different rows pays
// two scalar instructions and a lane read more than the plain form.
template <bool MERGE>
struct FragOne {
    const BsigKParams &P;
    uint32_t *hist;
    int glo, gn, lenbin;
    __device__ __forceinline__ void operator()(int p, int e, bool neg, bool rej, int tl, bool valid) const
    {
        const int a = tl < 0 ? -tl : tl;
        bool ok = valid & !rej & (a >= P.tf0) & (a <= P.tf1);
        const int offset = P.midpoint ? a >> 1 : 0;
        const int p5 = neg ? e - offset : p + offset;
        ok = ok & ((unsigned)(p5 - glo) < (unsigned)gn);
        // (P.div_magic / P.div_shift are lenbin's in a frag plan: its tiles are count tiles, whose binsize is not read)
        const uint32_t row = lenbin == 1 ? (uint32_t)a : __umulhi((uint32_t)a, P.div_magic) >> P.div_shift;
        if constexpr (MERGE) {
            const unsigned long long m = __ballot(ok);
            if (m == 0ull) return;                              // (uniform over the active lanes)
            const int leader = __ffsll((long long)m) - 1;
            const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)row, leader);
            const bool same = ok & (row == r0);
            const uint32_t n_same = (uint32_t)__popcll(__ballot(same));
            const bool lead = (int)__lane_id() == leader;
            if (ok & (!same | lead)) atomicAdd(&hist[row], same ? n_same : 1u);
        } else {
            if (ok) atomicAdd(&hist[row], 1u);
        }
    }
};

// LDS of one k_frag_tiles workgroup, in dwords: histogram | filter table (LTAB)
__host__ __device__ inline int frag_hist_dwords(int n_rows) { return (n_rows + 3) & ~3; }

// LTAB: the packed class's filter table is copied into LDS (as everywhere else); without, at the row cap, where the
// histogram alone fills the 64 KiB a workgroup may ask for, its 512 bytes are read from global memory
template <int NT, bool MERGE, bool LTAB>
__global__ __launch_bounds__(NT) void k_frag_tiles(const BsigWorkItem *__restrict__ items, const uint2 *__restrict__ runs,
                                                   unsigned long long *__restrict__ out, const uint2 *__restrict__ windows,
                                                   const BsigReadsDev R, const BsigKParams P, int n_rows, int lenbin)
{
    extern __shared__ __attribute__((aligned(16))) int32_t lds[];
    const int tid = threadIdx.x;
    uint32_t *hist = reinterpret_cast<uint32_t *>(lds);
    for (int v = tid; v < n_rows; v += NT) hist[v] = 0u;
    const uint8_t *ptab = P.ptab;
    if constexpr (LTAB) {
        uint8_t *lt = reinterpret_cast<uint8_t *>(lds + frag_hist_dwords(n_rows));
        build_ptab<NT>(lt, R, P, tid);
        ptab = lt;
    }
    const uint2 run = runs[blockIdx.x];
    __syncthreads();
#pragma unroll 1
    for (uint32_t t = run.x; t < run.y; ++t) {
        const BsigWorkItem w = items[t];
        uint2 win[BSIG_MAX_CLASSES], clip;
        PackedWin pk;
        load_windows<false>(R, P, BSIG_MODE_COUNT, w, items, windows, win, t, pk, clip);
        const FragOne<MERGE> one{P, hist, w.loc + w.c0, w.nc, lenbin};
        for_each_read<NT, 2, false>(R, P, win, pk.base, ptab, tid, one);
        if (pk.n_chunks > 1) packed_later_chunks<NT>(R, P, BSIG_MODE_COUNT, w, pk.n_chunks, clip, ptab, tid, one);
    }
    __syncthreads();
    for (int v = tid; v < n_rows; v += NT) {
        const uint32_t c = hist[v];
        if (c) atomicAdd(out + v, (unsigned long long)c);
    }
}

// ------------------------------------------------------------------------------------------
// V-plot over ranges of one width (bsig_plan_create_vplot)
// ------------------------------------------------------------------------------------------
// The joint table of the two reductions above it: row = fragment length / lenbin (k_frag_tiles' row), column = the
// fragment's position in its range / binsize (bamProfile's cell), summed over the ranges.  The tiles are a frag plan's:
// sub-intervals [loc + c0, loc + c0 + nc) of a range without an image, their windows reaching ext = tf1 under the
// midpoint rule, so the reads are streamed once whatever the table's size.  A workgroup owns a run of tiles.  A read
// that FragOne accepts lies at rel = p5 - loc in its range; a '-' range is mirrored first (rel = w - 1 - rel) and binned
// second, as ProfileOne does.  a and rel are below 2^31 and divided with magic_u31's multipliers at full width: lenbin's
// in P.div_magic / P.div_shift (a frag plan's), binsize's in the kernel's own arguments.  No 24-bit multiply touches a,
// a / 2 or rel: lengths reach 2^30.
// LDS form (GLOBAL = false): every range has the same width, so ONE table of n_rows x n_cols 32-bit counters in LDS
// serves every tile of the run; the plan cuts the runs so that the reads in a run's windows stay below 2^32
// (runtime.hip: vplot_setup), and the run ends with one 64-bit global atomic per non-zero cell.  The filter table sits
// behind the counters where the two fit the budget (LTAB), else it is read from global memory.
// Global form (GLOBAL = true): a table beyond the LDS budget; every accepted read adds 1 to its int64 cell of the result
// with a 64-bit global atomic whose value nobody reads.  No counter can wrap.
// MERGE (either form; FragOne<true>'s scheme on the cell): the lanes that hold the cell of the wave's first accepted lane
// are counted with a ballot and added by that lane alone, the other cells take their own atomics.  A pile of duplicates
// then costs one atomic a wave instead of 64; a wave of all-different cells pays two scalar instructions and a lane read
// more.  The plain forms are the default: runtime.hip (vplot_setup) says what was measured.
template <bool GLOBAL, bool MERGE>
struct VplotOne {
    const BsigKParams &P;
    uint32_t *tab;                      // LDS form: the run's table
    unsigned long long *out;            // global form: the result
    int loc, w1, c0, nc;                // the range's start and width - 1; the tile's bases [c0, c0 + nc) of the range
    int lenbin, binsize, n_cols;
    uint32_t bin_magic;
    int bin_shift;
    bool neg_range;
    __device__ __forceinline__ void operator()(int p, int e, bool neg, bool rej, int tl, bool valid) const
    {
        const int a = tl < 0 ? -tl : tl;
        bool ok = valid & !rej & (a >= P.tf0) & (a <= P.tf1);
        const int offset = P.midpoint ? a >> 1 : 0;
        const int p5 = neg ? e - offset : p + offset;
        int rel = p5 - loc;
        ok = ok & ((unsigned)(rel - c0) < (unsigned)nc);
        rel = neg_range ? w1 - rel : rel;
        const uint32_t col = binsize == 1 ? (uint32_t)rel : __umulhi((uint32_t)rel, bin_magic) >> bin_shift;
        const uint32_t row = lenbin == 1 ? (uint32_t)a : __umulhi((uint32_t)a, P.div_magic) >> P.div_shift;
        // (ok: tf0 <= a <= tf1 and 0 <= rel < w, so row < n_rows and col < n_cols: cell < 2^24)
        const uint32_t cell = row * (uint32_t)n_cols + col;
        uint32_t n = 1u;
        if constexpr (MERGE) {
            const unsigned long long m = __ballot(ok);
            if (m == 0ull) return;                              // (uniform over the active lanes)
            const int leader = __ffsll((long long)m) - 1;
            const uint32_t first = (uint32_t)__builtin_amdgcn_readlane((int)cell, leader);
            const bool same = ok & (cell == first);
            n = same ? (uint32_t)__popcll(__ballot(same)) : 1u;
            ok = ok & (!same | ((int)__lane_id() == leader));
        }
        if (!ok) return;
        if constexpr (GLOBAL) atomicAdd(out + cell, (unsigned long long)n);
        else atomicAdd(&tab[cell], n);
    }
};

// LDS of one k_vplot_tiles workgroup, in dwords: table (LDS form) | filter table (LTAB)
__host__ __device__ inline int vplot_tab_dwords(bool global, int n_cells) { return global ? 0 : (n_cells + 3) & ~3; }

template <int NT, bool GLOBAL, bool LTAB, bool MERGE>
__global__ __launch_bounds__(NT) void k_vplot_tiles(const BsigWorkItem *__restrict__ items, const uint2 *__restrict__ runs,
                                                    unsigned long long *__restrict__ out, const uint2 *__restrict__ windows,
                                                    const BsigReadsDev R, const BsigKParams P, int n_rows, int n_cols, int lenbin,
                                                    int binsize, uint32_t bin_magic, int bin_shift)
{
    extern __shared__ __attribute__((aligned(16))) int32_t lds[];
    const int tid = threadIdx.x;
    const int n_cells = n_rows * n_cols;
    uint32_t *tab = reinterpret_cast<uint32_t *>(lds);
    if constexpr (!GLOBAL)
        for (int v = tid; v < n_cells; v += NT) tab[v] = 0u;
    const uint8_t *ptab = P.ptab;
    if constexpr (LTAB) {
        uint8_t *lt = reinterpret_cast<uint8_t *>(lds + vplot_tab_dwords(GLOBAL, n_cells));
        build_ptab<NT>(lt, R, P, tid);
        ptab = lt;
    }
    const uint2 run = runs[blockIdx.x];
    __syncthreads();
#pragma unroll 1
    for (uint32_t t = run.x; t < run.y; ++t) {
        const BsigWorkItem w = items[t];
        uint2 win[BSIG_MAX_CLASSES], clip;
        PackedWin pk;
        load_windows<false>(R, P, BSIG_MODE_COUNT, w, items, windows, win, t, pk, clip);
        const VplotOne<GLOBAL, MERGE> one{P, tab, out, w.loc, w.len - 1, w.c0, w.nc, lenbin, binsize, n_cols, bin_magic, bin_shift,
                                   (w.units_strand & BSIG_ITEM_NEG) != 0u};
        for_each_read<NT, 2, false>(R, P, win, pk.base, ptab, tid, one);
        if (pk.n_chunks > 1) packed_later_chunks<NT>(R, P, BSIG_MODE_COUNT, w, pk.n_chunks, clip, ptab, tid, one);
    }
    if constexpr (!GLOBAL) {
        __syncthreads();
        for (int v = tid; v < n_cells; v += NT) {
            const uint32_t c = tab[v];
            if (c) atomicAdd(out + v, (unsigned long long)c);
        }
    }
}

// ------------------------------------------------------------------------------------------
// Depth histogram over ranges (bsig_plan_create_hist)
// ------------------------------------------------------------------------------------------
// A tile is up to P.tile_cells consecutive cells of one range, as an ordinary per-base tile is, and writes no per-range
// cell.  A workgroup owns a run of tiles and keeps ONE histogram of n_rows = V + 1 32-bit counters in LDS for all of
// them.  Per tile it builds the image the ordinary kernels build -- 5' ends per strand (ProfileOne<true>: dword x holds
// sense[x] in its low half and antisense[x] in its high half; with P.ss every half is a cell, without the cell is their
// sum), or coverage's signed 16-bit difference image (CoverOne) followed by k_coverage's workgroup prefix scan -- and
// then counts the tile's cells by value: row min(value, V) += 1, and the true value into the lane's 64-bit sum.  A lane
// clears the image cells it has just read, so the tile ends with one barrier.  Cells of the image behind the tile's nc
// are never counted.
// WIDE (tiles with more reads in their windows than a 16-bit cell may see, which the plan lists apart; they cannot be
// cut into slices, because a cell's value must be complete before it is counted): 32-bit image cells, read by read.
// Exactness.  Every cell adds 1 to one counter and the plan ends a run before its cells pass 2^32 - 1 (runtime.hip:
// hist_setup); the plan bounds the sum moment below 2^63.  At the end of its run a workgroup adds its non-zero rows to
// the int64 result with one 64-bit atomic each and its sum with one per wave.
// Contention.  EVERY cell of a tile goes to the histogram, and on sparse data nearly all of them to row 0 -- one LDS
// address, which the LDS serves one lane per cycle.  FORM 0 (plain): one LDS atomic per cell.  FORM 1 (merge): the zero
// cells of a wave are counted by ballot into a scalar that the wave adds to row 0 once per tile; of the others, the lanes
// that hold the row of the wave's first such lane are counted with a second ballot and added by that lane alone
// (FragOne<true>'s scheme), the rest add for themselves.
enum { kHistEnds = 0, kHistEndsHalf = 1, kHistCover = 2 };

// the read-by-read body of a WIDE coverage tile: an int32 difference image
struct CoverWideOne {
    const BsigKParams &P;
    int32_t *img;
    int loc, c0, nc;
    bool neg_range;
    int rend1;
    __device__ __forceinline__ void operator()(int p, int e, bool neg, bool rej, int tl, bool valid) const
    {
        if (!valid || rej || tlen_rejected(P, tl)) return;
        int start, end;
        covered_interval<false>(P, p, e, neg, tl, start, end);       // (no reduction takes a resized plan yet)
        const int ra = neg_range ? rend1 - end : start - loc;
        const int rb = neg_range ? rend1 - start : end - loc;
        const int la = ra - c0, lb = rb - c0;
        if (la >= nc || lb < 0) return;
        atomicAdd(&img[la > 0 ? la : 0], 1);
        if (lb + 1 < nc) atomicAdd(&img[lb + 1], -1);
    }
};

// LDS of one k_hist_tiles workgroup, in dwords: image | scan totals | filter table | histogram
struct HistLds {
    int img, wtot, ptab, hist, total;
};
__host__ __device__ inline int hist_img_dwords(int kind, bool wide, int tile_cells)
{
    // coverage: whole 16-B vectors of four cells a lane (16-bit: 8-B pairs of dwords, four cells); ends: a dword per cell,
    // two with 32-bit cells
    if (kind == kHistCover) return wide ? (tile_cells + 3) & ~3 : ((tile_cells + 3) / 4 * 2 + 3) & ~3;
    return ((wide ? 2 : 1) * tile_cells + 3) & ~3;
}
__host__ __device__ inline HistLds hist_lds(int kind, bool wide, int tile_cells, int n_rows)
{
    HistLds L;
    L.img = 0;
    L.wtot = hist_img_dwords(kind, wide, tile_cells);
    L.ptab = L.wtot + 4;
    L.hist = L.ptab + BSIG_PACK_CODES / 4;
    L.total = L.hist + ((n_rows + 3) & ~3);
    return L;
}

template <int FORM>
struct HistCounter {
    uint32_t *hist;
    uint32_t top;                       // V: the overflow row
    uint32_t zeros = 0;                 // FORM 1: the wave's zero cells of this tile (uniform over the wave)
    unsigned long long sum = 0;
    // (called by all lanes of a wave together: the loops around it are uniform)
    __device__ __forceinline__ void operator()(uint32_t v, bool ok)
    {
        sum += ok ? v : 0u;
        const uint32_t row = v < top ? v : top;
        if constexpr (FORM == 1) {
            const bool z = ok & (v == 0u);
            zeros += (uint32_t)__popcll(__ballot(z));
            const bool rest = ok & !z;
            const unsigned long long m = __ballot(rest);
            if (m == 0ull) return;                              // (uniform)
            const int leader = __ffsll((long long)m) - 1;
            const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)row, leader);
            const bool same = rest & (row == r0);
            const uint32_t n_same = (uint32_t)__popcll(__ballot(same));
            const bool lead = (int)__lane_id() == leader;
            if (rest & (!same | lead)) atomicAdd(&hist[row], same ? n_same : 1u);
        } else {
            if (ok) atomicAdd(&hist[row], 1u);
        }
    }
    // walk_tile_cells' consumer: the histogram asks neither for the cell's place nor for its strand
    template <int ROW>
    __device__ __forceinline__ void at(uint32_t v, bool ok, int) { (*this)(v, ok); }
    // once per tile
    __device__ __forceinline__ void flush_zeros()
    {
        if constexpr (FORM == 1) {
            if (zeros && __lane_id() == 0) atomicAdd(&hist[0], zeros);
            zeros = 0;
        }
    }
};

// The walk k_hist_tiles and k_summary_tiles share: tile w's image is built in `img` (which arrives zeroed) by the existing
// read bodies, coverage's difference image is scanned, and every cell goes to the consumer ONCE, as
// cnt.at<ROW>(value, ok, x): x the cell's index in the tile (range orientation; lanes take ascending x within a call and
// from call to call), ok whether x < nc (a cell behind the tile is handed over with ok false and no meaning), ROW 1 the
// antisense cell of a strand-split tile and 0 everything else.  All lanes of a wave call it together.  A lane clears the
// image cells it has read; the caller's barrier ends the tile.
template <int NT, int KIND, bool WIDE, typename Cells>
__device__ __forceinline__ void walk_tile_cells(const BsigWorkItem &w, uint32_t t, const BsigWorkItem *__restrict__ items,
                                                const uint2 *__restrict__ windows, const BsigReadsDev &R, const BsigKParams &P,
                                                uint32_t *img, int32_t *wtot, const uint8_t *ptab, int tid, Cells &cnt)
{
    const int lane = tid & (kWave - 1);
    uint2 win[BSIG_MAX_CLASSES], clip;
    PackedWin pk;
    const bool neg_range = (w.units_strand & BSIG_ITEM_NEG) != 0u;
    const int nc = w.nc;
    if constexpr (KIND == kHistCover) {
        load_windows<false>(R, P, BSIG_MODE_COVERAGE, w, items, windows, win, t, pk, clip);
        const int rend1 = w.loc + w.len - 1;
        if constexpr (WIDE) {
            const CoverWideOne one{P, reinterpret_cast<int32_t *>(img), w.loc, w.c0, nc, neg_range, rend1};
            for_each_read<NT, 2, false>(R, P, win, pk.base, ptab, tid, one);
            if (pk.n_chunks > 1) packed_later_chunks<NT>(R, P, BSIG_MODE_COVERAGE, w, pk.n_chunks, clip, ptab, tid, one);
        } else {
            const CoverOne one{P, reinterpret_cast<int32_t *>(img), w.loc, w.c0, nc, 0, neg_range, rend1};
            for_each_read<NT, 2, false>(R, P, win, pk.base, ptab, tid, one);
            if (pk.n_chunks > 1) packed_later_chunks<NT>(R, P, BSIG_MODE_COVERAGE, w, pk.n_chunks, clip, ptab, tid, one);
        }
        __syncthreads();
        // k_coverage's scan: each lane owns 4 consecutive cells, wave scan of the lane totals, carry across waves
        // and passes; the cells are handed over instead of stored
        const int nvec = (nc + 3) >> 2;
        auto lo16 = [](uint32_t d) { return (int)(int16_t)(uint16_t)d; };
        auto hi16 = [](uint32_t d) { return (int)(int16_t)(uint16_t)((d + 0x8000u) >> 16); };
        int carry = 0;
        for (int base = 0; base < nvec; base += NT) {
            const int v = base + tid;
            int4 x = make_int4(0, 0, 0, 0);
            if (v < nvec) {
                if constexpr (WIDE) {
                    int4 *p4 = reinterpret_cast<int4 *>(img) + v;
                    x = *p4;
                    *p4 = make_int4(0, 0, 0, 0);
                } else {
                    uint2 *p2 = reinterpret_cast<uint2 *>(img) + v;
                    const uint2 d = *p2;
                    *p2 = make_uint2(0u, 0u);
                    x = make_int4(lo16(d.x), hi16(d.x), lo16(d.y), hi16(d.y));
                }
            }
            x.y += x.x; x.z += x.y; x.w += x.z;
            const int tot = x.w;
            const int incl = wave_inclusive_scan(tot);
            int pre = carry;
            int all = __builtin_amdgcn_readlane(incl, kWave - 1);
            if (NT > kWave) {
                if (lane == kWave - 1) wtot[tid / kWave] = incl;
                __syncthreads();
                all = 0;
                for (int k = 0; k < NT / kWave; ++k) {
                    const int s = wtot[k];
                    if (k < tid / kWave) pre += s;
                    all += s;
                }
                __syncthreads();
            }
            const int add = pre + incl - tot;
            const int c = 4 * v;
            cnt.template at<0>((uint32_t)(x.x + add), c < nc, c);
            cnt.template at<0>((uint32_t)(x.y + add), c + 1 < nc, c + 1);
            cnt.template at<0>((uint32_t)(x.z + add), c + 2 < nc, c + 2);
            cnt.template at<0>((uint32_t)(x.w + add), c + 3 < nc, c + 3);
            carry += all;
        }
    } else {
        load_windows<false>(R, P, BSIG_MODE_PROFILE, w, items, windows, win, t, pk, clip);
        if constexpr (WIDE && wants_shift<Cells>::value) {
            const ShiftedWideOne one{P, img, w.loc, w.len, w.c0, nc, neg_range};
            for_each_read<NT, 2, false>(R, P, win, pk.base, ptab, tid, one);
            if (pk.n_chunks > 1) packed_later_chunks<NT>(R, P, BSIG_MODE_PROFILE, w, pk.n_chunks, clip, ptab, tid, one);
        } else if constexpr (WIDE) {
            const XcorrWideOne one{P, img, w.loc, w.len, w.c0, nc, neg_range};
            for_each_read<NT, 2, false>(R, P, win, pk.base, ptab, tid, one);
            if (pk.n_chunks > 1) packed_later_chunks<NT>(R, P, BSIG_MODE_PROFILE, w, pk.n_chunks, clip, ptab, tid, one);
        } else {
            constexpr bool HALF = KIND == kHistEndsHalf;
            const ProfileOne<true> one{P, img, w.loc, w.len, w.c0, nc, 0, neg_range};
            for_each_read<NT, 2, HALF>(R, P, win, pk.base, ptab, tid, one);
            if (!HALF && pk.n_chunks > 1) packed_later_chunks<NT>(R, P, BSIG_MODE_PROFILE, w, pk.n_chunks, clip, ptab, tid, one);
        }
        __syncthreads();
        const bool ss = P.ss != 0;                                  // (uniform)
        for (int base = 0; base < nc; base += NT) {
            const int x = base + tid;
            const bool ok = x < nc;
            uint32_t s = 0, a = 0;
            if (ok) {
                if constexpr (WIDE) {
                    uint2 *p2 = reinterpret_cast<uint2 *>(img) + x;
                    const uint2 d = *p2;
                    *p2 = make_uint2(0u, 0u);
                    s = d.x; a = d.y;
                } else {
                    const uint32_t d = img[x];
                    img[x] = 0u;
                    s = d & 0xFFFFu; a = d >> 16;
                }
            }
            if (ss) { cnt.template at<0>(s, ok, x); cnt.template at<1>(a, ok, x); }
            else cnt.template at<0>(s + a, ok, x);
        }
    }
}

template <int NT, int KIND, bool WIDE, int FORM>
__global__ __launch_bounds__(NT) void k_hist_tiles(const BsigWorkItem *__restrict__ items, const uint2 *__restrict__ runs,
                                                   unsigned long long *__restrict__ out, const uint2 *__restrict__ windows,
                                                   const BsigReadsDev R, const BsigKParams P, int n_rows,
                                                   unsigned long long n_cells)
{
    static_assert(!(WIDE && KIND == kHistEndsHalf), "a wide tile reads the packed words");
    extern __shared__ __attribute__((aligned(16))) int32_t lds[];
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const HistLds L = hist_lds(KIND, WIDE, P.tile_cells, n_rows);
    uint32_t *img = reinterpret_cast<uint32_t *>(lds) + L.img;
    int32_t *wtot = lds + L.wtot;
    uint8_t *ptab = reinterpret_cast<uint8_t *>(lds + L.ptab);
    uint32_t *hist = reinterpret_cast<uint32_t *>(lds) + L.hist;
    for (int v = tid; v < L.ptab; v += NT) lds[v] = 0;
    for (int v = tid; v < n_rows; v += NT) hist[v] = 0u;
    if (KIND != kHistEndsHalf) build_ptab<NT>(ptab, R, P, tid);
    const uint2 run = runs[blockIdx.x];
    HistCounter<FORM> cnt{hist, (uint32_t)(n_rows - 1)};
    __syncthreads();

#pragma unroll 1
    for (uint32_t t = run.x; t < run.y; ++t) {
        const BsigWorkItem w = items[t];
        // (a tile listed apart for the wide launch: its cells are counted there, none here)
        if (!WIDE && (w.units_strand & BSIG_ITEM_HEAVY)) continue;
        walk_tile_cells<NT, KIND, WIDE>(w, t, items, windows, R, P, img, wtot, ptab, tid, cnt);
        cnt.flush_zeros();
        __syncthreads();
    }
    __syncthreads();
    for (int v = tid; v < n_rows; v += NT) {
        const uint32_t c = hist[v];
        if (c) atomicAdd(out + v, (unsigned long long)c);
    }
    unsigned long long m_sum = cnt.sum;
    for (int m = kWave / 2; m >= 1; m /= 2) m_sum += __shfl_xor(m_sum, m);
    if (lane == 0) {
        unsigned long long *mo = out + n_rows;                  // moments: [cells (the plan's count), sum of the values]
        if (blockIdx.x == 0 && tid == 0 && n_cells) atomicAdd(mo, n_cells);
        if (m_sum) atomicAdd(mo + 1, m_sum);
    }
}

// ------------------------------------------------------------------------------------------
// Per-range summaries (bsig_plan_create_summary)
// ------------------------------------------------------------------------------------------
// The first kind that reduces every range BY ITSELF: per (range, row) the sum of the per-base cells, their maximum, the
// first cell that holds it, and the number of cells at or above each of K thresholds.  Tiles, images and the scan are the
// depth histogram's (walk_tile_cells); the tile's work item carries the result row of its range (out_off = range x S).
// Consumer.  A lane keeps per row a 64-bit sum, a 64-bit key value << 32 | (2^32 - 1 - cell) -- the largest key is the
// largest value at the smallest cell, and a cell that exists has a key above 0 -- and one 32-bit counter per threshold.
// The thresholds are kernel arguments and stay in SGPRs.  Counters per lane, not ballot + popcount: read off the ISA, a
// counter costs v_cmp_le_u32 + v_addc_co_u32 a cell (two VALU), the ballot form v_cmp + s_bcnt1_i32_b64 + s_add_u32 with
// the K x S running counts wave-uniform -- and these kernels already sit at the SGPR ceiling with dozens of SGPRs spilled
// into VGPR lanes (the walk's windows and read columns), so every such count would live in a spill lane and pay a
// v_readlane / v_writelane pair per cell step.  VGPRs are free here.  Thresholds past K are 2^32 - 1, and their counters
// are never written out.
// Combining.  A workgroup owns a run of consecutive tiles; a range's tiles are consecutive.  The lanes carry their
// accumulators from tile to tile while the row is the same.  When it changes, or the run ends, the workgroup flushes:
// shuffle reduction in the wave, lane 0 of every wave into 2 + K LDS qwords per row (ds_add_u64 / ds_max_u64), then one
// 64-bit global atomic per non-zero qword into the range's row -- add for sum and counts, max for the key -- because a
// range may straddle runs and the wide launch.  A whole-chromosome range costs 2 + K atomics per run per row.
// Exactness.  A lane's counter grows by at most the cells of its run, which the plan keeps below 2^32 (summary_setup);
// the plan proves every range's sum below 2^63.  k_summary_finish turns the key into max and summit.
struct SummaryCells {
    const BsigThresholds &T;
    uint32_t c0 = 0;                                    // the tile's first cell in its range
    unsigned long long sum[2] = {0ull, 0ull}, key[2] = {0ull, 0ull};
    uint32_t cnt[2][BSIG_SUMMARY_MAX_THRESHOLDS] = {};
    template <int ROW>
    __device__ __forceinline__ void at(uint32_t v, bool ok, int x)
    {
        v = ok ? v : 0u;
        sum[ROW] += v;
        const unsigned long long k = ok ? ((unsigned long long)v << 32) | (0xFFFFFFFFu - (c0 + (uint32_t)x)) : 0ull;
        key[ROW] = k > key[ROW] ? k : key[ROW];
#pragma unroll
        for (int j = 0; j < BSIG_SUMMARY_MAX_THRESHOLDS; ++j) cnt[ROW][j] += v >= T.t[j] ? 1u : 0u;
    }
    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            sum[r] = 0ull; key[r] = 0ull;
#pragma unroll
            for (int j = 0; j < BSIG_SUMMARY_MAX_THRESHOLDS; ++j) cnt[r][j] = 0u;
        }
    }
};

// LDS of one k_summary_tiles workgroup: the histogram kernel's, with the flush's qwords (kSummarySlots per row, two rows)
// where its histogram is
constexpr int kSummarySlots = 2 + BSIG_SUMMARY_MAX_THRESHOLDS;       // sum | key | counts
__host__ __device__ inline HistLds summary_lds(int kind, bool wide, int tile_cells)
{
    return hist_lds(kind, wide, tile_cells, 2 * 2 * kSummarySlots);
}

template <int NT, int KIND, bool WIDE>
__global__ __launch_bounds__(NT) void k_summary_tiles(const BsigWorkItem *__restrict__ items, const uint2 *__restrict__ runs,
                                                      unsigned long long *__restrict__ out, const uint2 *__restrict__ windows,
                                                      const BsigReadsDev R, const BsigKParams P, const BsigThresholds T)
{
    static_assert(!(WIDE && KIND == kHistEndsHalf), "a wide tile reads the packed words");
    extern __shared__ __attribute__((aligned(16))) int32_t lds[];
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const HistLds L = summary_lds(KIND, WIDE, P.tile_cells);
    uint32_t *img = reinterpret_cast<uint32_t *>(lds) + L.img;
    int32_t *wtot = lds + L.wtot;
    uint8_t *ptab = reinterpret_cast<uint8_t *>(lds + L.ptab);
    unsigned long long *slot = reinterpret_cast<unsigned long long *>(lds + L.hist);      // (16-byte aligned: hist_lds)
    for (int v = tid; v < L.ptab; v += NT) lds[v] = 0;
    for (int v = tid; v < 2 * kSummarySlots; v += NT) slot[v] = 0ull;
    if (KIND != kHistEndsHalf) build_ptab<NT>(ptab, R, P, tid);
    const uint2 run = runs[blockIdx.x];
    const int K = T.k;
    const int S = KIND != kHistCover && P.ss ? 2 : 1;                 // (uniform)
    const int stride = BSIG_SUMMARY_FIXED + K;                        // int64 per (range, row) of the result
    SummaryCells cnt{T};
    __syncthreads();

    // the lanes' accumulators into result row `row0` (and row0 + 1 with strands), and cleared; uniform over the workgroup
    // (the row is a compile-time index, so that the accumulators stay in registers)
    auto flush_row = [&](auto row) {
        constexpr int r = decltype(row)::value;
        unsigned long long s = cnt.sum[r], k = cnt.key[r];
        for (int m = kWave / 2; m >= 1; m /= 2) {
            s += __shfl_xor(s, m);
            const unsigned long long o = __shfl_xor(k, m);
            k = o > k ? o : k;
        }
        if (lane == 0) {
            if (s) atomicAdd(&slot[r * kSummarySlots], s);
            atomicMax(&slot[r * kSummarySlots + 1], k);
        }
#pragma unroll
        for (int j = 0; j < BSIG_SUMMARY_MAX_THRESHOLDS; ++j) {
            if (j >= K) break;                                    // (uniform)
            uint32_t c = cnt.cnt[r][j];
            for (int m = kWave / 2; m >= 1; m /= 2) c += __shfl_xor(c, m);
            if (lane == 0 && c) atomicAdd(&slot[r * kSummarySlots + 2 + j], (unsigned long long)c);
        }
    };
    auto flush = [&](long long row0) {
        flush_row(std::integral_constant<int, 0>{});
        if constexpr (KIND != kHistCover) {
            if (S == 2) flush_row(std::integral_constant<int, 1>{});
        }
        __syncthreads();
        if (tid < 2 * kSummarySlots) {
            const int r = tid / kSummarySlots, f = tid - r * kSummarySlots;
            if (r < S && f < 2 + K) {
                const unsigned long long v = slot[tid];
                slot[tid] = 0ull;
                unsigned long long *dst = out + (size_t)(row0 + r) * (size_t)stride + (f < 2 ? f : f + 1);
                if (f == 1) { if (v) atomicMax(dst, v); }
                else if (v) atomicAdd(dst, v);
            }
        }
        __syncthreads();
        cnt.clear();
    };

    long long cur = -1;
#pragma unroll 1
    for (uint32_t t = run.x; t < run.y; ++t) {
        const BsigWorkItem w = items[t];
        // (a tile listed apart for the wide launch: its cells are summed up there, none here)
        if (!WIDE && (w.units_strand & BSIG_ITEM_HEAVY)) continue;
        if (w.out_off != cur) {
            if (cur >= 0) flush(cur);
            cur = w.out_off;
        }
        cnt.c0 = (uint32_t)w.c0;
        walk_tile_cells<NT, KIND, WIDE>(w, t, items, windows, R, P, img, wtot, ptab, tid, cnt);
        __syncthreads();
    }
    if (cur >= 0) flush(cur);
}

// One thread per (range, row): the key at [1] becomes the maximum at [1] and the summit at [2] -- -1 where no cell was
// seen (key 0: a range without width).  The rows already lie in the caller's order.
__global__ __launch_bounds__(256) void k_summary_finish(long long *__restrict__ out, long long n_rows, int stride)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_rows) return;
    long long *row = out + i * stride;
    const unsigned long long key = (unsigned long long)row[1];
    row[1] = (long long)(key >> 32);
    row[2] = key ? (long long)(0xFFFFFFFFu - (uint32_t)key) : -1ll;
}

// ------------------------------------------------------------------------------------------
// Scaled regions (bsig_plan_create_scaled)
// ------------------------------------------------------------------------------------------
// Every range cut into the same number N of bins whatever its width w: cell c of the range (range orientation) belongs to
// bin floor(c * N / w), and every (range, row) receives the N sums of its bins' cells.  Tiles, images, the scan and the
// work item's result row (out_off = range x S) are the summaries' (walk_tile_cells); a result row is N int64.
// Bin index.  No 64-bit division per cell.  Once per tile, uniform over the workgroup: c0 * N = q0 * w + r0 (one 64-bit
// division, none for a range's first tile).  Cell x of the tile then lies in bin q0 + floor(u / w), u = r0 + x * N.  With
// x < 2,048 and N <= 2,048, u < w + 2^22: it fits 32 bits unsigned, but not 31.  Two exact forms, chosen by the uniform w:
//   w >= 2^23: u < 2 w, so the quotient is u >= w.
//   w <  2^23: u < 2^24 is exact as a float, and so is w.  q' = trunc(float(u) * (1 / float(w))) with the reciprocal
//     rounded to nearest (1 / w below is IEEE division) and the product rounded once: the relative error is below 2^-23 and
//     the quotient below 1 + 2^22, so q' is floor(u / w) - 1, floor(u / w) or floor(u / w) + 1, and the remainder
//     u - q' w, which fits 32 bits signed (q' w < 2^25), says which: one fix-up step down, one up.
// The bin is clamped to N - 1, which an exact quotient never needs (c < w): no address depends on the arithmetic being right.
// Accumulation.  S * N 64-bit accumulators in LDS.  Plain form: one ds_add_u64 per non-zero cell.  Within a call of `at`
// lanes take ascending x, so the bins do not decrease across the wave and a bin is a contiguous run of lanes.  Segmented
// form (SEG; 16-bit images only): a wave whose 64 cells lie in ONE bin -- where the plain form puts 64 lanes on one LDS
// address; the 64 cells of a call are neighbours for 5' ends (the rule from w / N >= 64 on) and four apart for coverage,
// where a lane owns four consecutive cells (w / N >= 256) -- adds them up with xor shuffles and issues one LDS add; any
// other wave runs a segmented inclusive scan keyed on the bin (shuffle up by 1, 2, .. 32; a lane adds while the lane that
// far below holds its bin) and the last lane of every bin adds the bin's sum.  The plan picks the form (runtime.hip: scaled_setup).
// Combining.  As in k_summary_tiles: a workgroup carries its accumulators while out_off stays the same and flushes when it
// changes and when the run ends, one 64-bit global atomic add per non-zero accumulator into out[row * N + j], because a
// range may straddle runs and the wide launch.  The flush visits the bins [lo, hi] the tiles since the last flush touched:
// an interval, since those tiles are neighbours in one range, and uniform over the workgroup.
// Exactness.  Nothing is narrower than 64 bits but the segmented form's 32-bit wave sums: 64 cells of a 16-bit image, each
// at most 2 * 65,535 (both strands of a 5'-end cell), stay below 2^23.  A wide tile takes the plain form.  The plan proves
// every range's sum below 2^63 (the summaries' proof).
template <bool SEG>
struct ScaledCells {
    unsigned long long *acc;            // LDS: S rows of N accumulators
    uint32_t N;
    int lane;
    uint32_t w = 1u, q0 = 0u, r0 = 0u;  // the tile's range width; c0 * N = q0 * w + r0
    float rcp = 1.f;                    // 1 / w
    // once per tile, uniform
    __device__ __forceinline__ void tile(const BsigWorkItem &t)
    {
        w = (uint32_t)t.len;
        rcp = 1.0f / (float)w;
        q0 = 0u; r0 = 0u;
        if (t.c0 != 0) {
            const unsigned long long p = (unsigned long long)(uint32_t)t.c0 * N;
            q0 = (uint32_t)(p / w);
            r0 = (uint32_t)(p - (unsigned long long)q0 * w);
        }
    }
    __device__ __forceinline__ uint32_t bin(uint32_t x) const
    {
        const uint32_t u = r0 + x * N;
        uint32_t q;
        if (w >= (1u << 23)) {                                      // (uniform)
            q = u >= w ? 1u : 0u;
        } else {
            q = (uint32_t)((float)u * rcp);
            int32_t r = (int32_t)(u - q * w);
            if (r < 0) { --q; r += (int32_t)w; }
            if (r >= (int32_t)w) ++q;
        }
        const uint32_t b = q0 + q;
        return b < N ? b : N - 1u;
    }
    template <int ROW>
    __device__ __forceinline__ void at(uint32_t v, bool ok, int x)
    {
        if constexpr (!SEG) {
            if (ok && v) atomicAdd(&acc[ROW * N + bin((uint32_t)x)], (unsigned long long)v);
        } else {
            // (all lanes of the wave are here: the loops around the call are uniform)
            const uint32_t b = ok ? bin((uint32_t)x) : 0xFFFFFFFFu;
            uint32_t s = ok ? v : 0u;
            const uint32_t b_first = (uint32_t)__builtin_amdgcn_readfirstlane((int)b);
            const uint32_t b_last = (uint32_t)__builtin_amdgcn_readlane((int)b, kWave - 1);
            if (b_first == b_last) {                                // (uniform) one bin, or no cell at all
                if (b_first == 0xFFFFFFFFu) return;
                for (int m = kWave / 2; m >= 1; m /= 2) s += __shfl_xor(s, m);
                if (lane == 0 && s) atomicAdd(&acc[ROW * N + b], (unsigned long long)s);
                return;
            }
#pragma unroll
            for (int d = 1; d < kWave; d *= 2) {
                const uint32_t os = __shfl_up(s, d), ob = __shfl_up(b, d);
                if (lane >= d && ob == b) s += os;
            }
            const uint32_t nb = __shfl_down(b, 1);
            if (ok && s && (lane == kWave - 1 || nb != b)) atomicAdd(&acc[ROW * N + b], (unsigned long long)s);
        }
    }
};

// LDS of one k_scaled_tiles workgroup: the histogram kernel's, with rows * n_bins qwords where its histogram is
__host__ __device__ inline HistLds scaled_lds(int kind, bool wide, int tile_cells, int rows, int n_bins)
{
    return hist_lds(kind, wide, tile_cells, 2 * rows * n_bins);
}

template <int NT, int KIND, bool WIDE, bool SEG>
__global__ __launch_bounds__(NT) void k_scaled_tiles(const BsigWorkItem *__restrict__ items, const uint2 *__restrict__ runs,
                                                     unsigned long long *__restrict__ out, const uint2 *__restrict__ windows,
                                                     const BsigReadsDev R, const BsigKParams P, const int n_bins)
{
    static_assert(!(WIDE && KIND == kHistEndsHalf), "a wide tile reads the packed words");
    static_assert(!(WIDE && SEG), "the segmented form's wave sums are 32 bits wide: 16-bit images only");
    extern __shared__ __attribute__((aligned(16))) int32_t lds[];
    const int tid = threadIdx.x;
    const int S = KIND != kHistCover && P.ss ? 2 : 1;                 // (uniform)
    const HistLds L = scaled_lds(KIND, WIDE, P.tile_cells, S, n_bins);
    uint32_t *img = reinterpret_cast<uint32_t *>(lds) + L.img;
    int32_t *wtot = lds + L.wtot;
    uint8_t *ptab = reinterpret_cast<uint8_t *>(lds + L.ptab);
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(lds + L.hist);       // (16-byte aligned: hist_lds)
    for (int v = tid; v < L.ptab; v += NT) lds[v] = 0;
    for (int v = tid; v < S * n_bins; v += NT) acc[v] = 0ull;
    if (KIND != kHistEndsHalf) build_ptab<NT>(ptab, R, P, tid);
    const uint2 run = runs[blockIdx.x];
    ScaledCells<SEG> cnt{acc, (uint32_t)n_bins, tid & (kWave - 1)};
    __syncthreads();

    // the bins the tiles since the last flush touched (uniform), added into result row `row0` (and row0 + 1 with strands)
    int lo = n_bins, hi = -1;
    auto flush = [&](long long row0) {
        for (int r = 0; r < S; ++r) {
            for (int j = lo + tid; j <= hi; j += NT) {
                const unsigned long long v = acc[r * n_bins + j];
                if (v) {
                    acc[r * n_bins + j] = 0ull;
                    atomicAdd(out + (size_t)(row0 + r) * (size_t)n_bins + (size_t)j, v);
                }
            }
        }
        __syncthreads();
        lo = n_bins; hi = -1;
    };

    long long cur = -1;
#pragma unroll 1
    for (uint32_t t = run.x; t < run.y; ++t) {
        const BsigWorkItem w = items[t];
        // (a tile listed apart for the wide launch: its cells are binned there, none here)
        if (!WIDE && (w.units_strand & BSIG_ITEM_HEAVY)) continue;
        if (w.out_off != cur) {
            if (cur >= 0) flush(cur);
            cur = w.out_off;
        }
        cnt.tile(w);
        const int b0 = (int)(cnt.q0 < (uint32_t)n_bins ? cnt.q0 : (uint32_t)n_bins - 1u), b1 = (int)cnt.bin((uint32_t)(w.nc - 1));
        lo = b0 < lo ? b0 : lo;
        hi = b1 > hi ? b1 : hi;
        walk_tile_cells<NT, KIND, WIDE>(w, t, items, windows, R, P, img, wtot, ptab, tid, cnt);
        __syncthreads();
    }
    if (cur >= 0) flush(cur);
}

// ------------------------------------------------------------------------------------------
// Capped 5' ends (bsig_plan_create_capped)
// ------------------------------------------------------------------------------------------
// keepDup = k: every per-base, per-strand 5'-end cell e is replaced by min(e, k) BEFORE anything is binned or the strands
// are added.  Tiles, images and the walk are the depth histogram's (walk_tile_cells) with the image always strand-split
// (P.ss is 1 whatever the result's strands: the walk then hands the sense cell over as row 0 and the antisense cell as row 1
// of the same x, one after the other, to the same lane); the tile's work item carries the first result cell of its RANGE
// (out_off), and the result is int32 in bsig_layout's order for the call's bins and strands: cell 2 * bin + antisense with
// strands, bin without.
// BINNED false (bins of one base): the tile owns its cells and stores them, zeros included -- one 8-byte store a lane with
// strands (the layout's offsets are even then), one 4-byte store without.  Nothing is zeroed first and nothing is atomic.
// BINNED true (wider bins, and bamCount as one bin of 2^31 - 1 bases): cell c0 + x lies in bin (c0 + x) / binsize, an exact
// magic division (magic_u31).  Lanes take ascending x, so a bin is a run of lanes: a wave with no cell to add is done, one with
// a few lets them add for themselves; of the others a wave whose cells lie in one bin adds them up with xor shuffles and
// issues one LDS add, any other runs ScaledCells' segmented scan keyed on the bin and the last lane of every bin adds.  The accumulators are int32 in LDS, one per bin the tile touches (planmath.h: capped_tile_bins)
// and row; after the tile the non-zero ones are added into the result with int32 global atomics, because a bin may straddle
// tiles, runs and the wide launch: the call zeroes the result first.  Integers: the order does not matter.
// Exactness.  A wave sum is at most the reads of a tile's windows, below 2^32; no capped sum exceeds the uncapped one, so
// the result's int32 contract is bamProfile's.
template <bool BINNED>
struct CappedCells {
    static constexpr bool kShifted = true;
    uint32_t k;                         // keepDup
    bool ss;                            // the RESULT's strands (the image always has them)
    int lane;
    int32_t *dst = nullptr;             // !BINNED: the tile's first result cell
    uint32_t *acc = nullptr;            // BINNED: LDS, rows of n_acc accumulators
    int n_acc = 0;
    uint32_t c0 = 0u, b0 = 0u;          // BINNED: the tile's first cell and that cell's bin
    uint32_t magic = 0u;
    int shift = 0;
    uint32_t held = 0u;                 // the capped sense cell, until the antisense cell of the same x arrives
    __device__ __forceinline__ uint32_t bin(uint32_t c) const { return __umulhi(c, magic) >> shift; }
    // (all lanes of the wave are here: the loops around `at` are uniform)
    __device__ __forceinline__ void add(uint32_t *row, uint32_t b, uint32_t s, bool ok) const
    {
        // 5' ends are mostly zeros: a wave without a cell to add is done, and one with a few (at most kSparse of its 64
        // lanes) lets them add for themselves -- cheaper than the twelve shuffles of the scan (s is 0 where ok is false)
        constexpr int kSparse = 16;
        const unsigned long long some = __ballot(s != 0u);
        if (some == 0ull) return;                                   // (uniform)
        if (__popcll(some) <= kSparse) {                            // (uniform)
            if (s) atomicAdd(&row[b], s);
            return;
        }
        const uint32_t b_first = (uint32_t)__builtin_amdgcn_readfirstlane((int)b);
        const uint32_t b_last = (uint32_t)__builtin_amdgcn_readlane((int)b, kWave - 1);
        if (b_first == b_last) {                                    // (uniform) one bin, or no cell at all
            if (b_first == 0xFFFFFFFFu) return;
            for (int m = kWave / 2; m >= 1; m /= 2) s += __shfl_xor(s, m);
            if (lane == 0 && s) atomicAdd(&row[b], s);
            return;
        }
#pragma unroll
        for (int d = 1; d < kWave; d *= 2) {
            const uint32_t os = __shfl_up(s, d), ob = __shfl_up(b, d);
            if (lane >= d && ob == b) s += os;
        }
        const uint32_t nb = __shfl_down(b, 1);
        if (ok && s && (lane == kWave - 1 || nb != b)) atomicAdd(&row[b], s);
    }
    template <int ROW>
    __device__ __forceinline__ void at(uint32_t v, bool ok, int x)
    {
        const uint32_t c = v < k ? v : k;
        if constexpr (ROW == 0) {
            held = c;
        } else if constexpr (!BINNED) {
            if (ok) {
                if (ss) *reinterpret_cast<int2 *>(dst + 2 * (size_t)x) = make_int2((int)held, (int)c);
                else dst[x] = (int)(held + c);
            }
        } else {
            // the bin within the tile's own; clamped, which an exact quotient never needs: no address depends on it
            uint32_t b = 0xFFFFFFFFu;
            if (ok) {
                b = bin(c0 + (uint32_t)x) - b0;
                b = b < (uint32_t)n_acc ? b : (uint32_t)n_acc - 1u;
            }
            if (ss) {
                add(acc, b, ok ? held : 0u, ok);
                add(acc + n_acc, b, ok ? c : 0u, ok);
            } else {
                add(acc, b, ok ? held + c : 0u, ok);
            }
        }
    }
};

template <int NT, int KIND, bool WIDE, bool BINNED>
__global__ __launch_bounds__(NT) void k_capped_tiles(const BsigWorkItem *__restrict__ items, const uint2 *__restrict__ runs,
                                                     int32_t *__restrict__ out, const uint2 *__restrict__ windows,
                                                     const BsigReadsDev R, const BsigKParams P, const int keep_dup, const int ss_out,
                                                     const uint32_t bin_magic, const int bin_shift, const int n_acc)
{
    static_assert(KIND == kHistEnds || KIND == kHistEndsHalf, "capped cells are 5' ends");
    static_assert(!(WIDE && KIND == kHistEndsHalf), "a wide tile reads the packed words");
    extern __shared__ __attribute__((aligned(16))) int32_t lds[];
    const int tid = threadIdx.x;
    const int S = ss_out ? 2 : 1;                                     // (uniform)
    const HistLds L = hist_lds(KIND, WIDE, P.tile_cells, BINNED ? S * n_acc : 0);
    uint32_t *img = reinterpret_cast<uint32_t *>(lds) + L.img;
    int32_t *wtot = lds + L.wtot;
    uint8_t *ptab = reinterpret_cast<uint8_t *>(lds + L.ptab);
    uint32_t *acc = reinterpret_cast<uint32_t *>(lds) + L.hist;
    for (int v = tid; v < L.ptab; v += NT) lds[v] = 0;
    if (BINNED) for (int v = tid; v < S * n_acc; v += NT) acc[v] = 0u;
    if (KIND != kHistEndsHalf) build_ptab<NT>(ptab, R, P, tid);
    const uint2 run = runs[blockIdx.x];
    CappedCells<BINNED> cnt{(uint32_t)keep_dup, ss_out != 0, tid & (kWave - 1)};
    cnt.acc = acc; cnt.n_acc = n_acc; cnt.magic = bin_magic; cnt.shift = bin_shift;
    __syncthreads();

#pragma unroll 1
    for (uint32_t t = run.x; t < run.y; ++t) {
        const BsigWorkItem w = items[t];
        // (a tile listed apart for the wide launch: its cells are capped there, none here)
        if (!WIDE && (w.units_strand & BSIG_ITEM_HEAVY)) continue;
        int nb = 0;
        if constexpr (BINNED) {
            cnt.c0 = (uint32_t)w.c0;
            cnt.b0 = cnt.bin((uint32_t)w.c0);
            nb = (int)(cnt.bin((uint32_t)(w.c0 + w.nc - 1)) - cnt.b0) + 1;
            nb = nb < n_acc ? nb : n_acc;
        } else {
            cnt.dst = out + w.out_off + (long long)w.c0 * S;
        }
        walk_tile_cells<NT, KIND, WIDE>(w, t, items, windows, R, P, img, wtot, ptab, tid, cnt);
        __syncthreads();
        if constexpr (BINNED) {
            for (int r = 0; r < S; ++r) {
                for (int j = tid; j < nb; j += NT) {
                    const uint32_t v = acc[r * n_acc + j];
                    if (v) {
                        acc[r * n_acc + j] = 0u;
                        atomicAdd(out + w.out_off + (long long)(cnt.b0 + (uint32_t)j) * S + r, (int32_t)v);
                    }
                }
            }
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------------------------------
// one-time layout of the reads in HBM
// ------------------------------------------------------------------------------------------

// bam_endpos(b) - 1 (htslib): sum of M(0) D(2) N(3) =(7) X(8) lengths; 0x4 or empty -> 1 base.
__global__ void k_cigar_end(int64_t n, const int32_t *__restrict__ pos,
                            const uint16_t *__restrict__ flag,
                            const int64_t *__restrict__ cigar_off,
                            const uint32_t *__restrict__ cigar, int32_t *__restrict__ end_out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int64_t rlen = 0;
    if (!(flag[i] & 0x4)) {
        const int64_t k1 = cigar_off[i + 1];
        for (int64_t k = cigar_off[i]; k < k1; ++k) {
            const uint32_t c = cigar[k];
            const uint32_t op = c & 0xFu;
            if ((0x18Du >> op) & 1u) rlen += c >> 4;    // bits 0,2,3,7,8
        }
    }
    if (rlen == 0) rlen = 1;
    end_out[i] = (int32_t)(pos[i] + rlen - 1);
}

// Span classes 0 and 1 keep `span - 1` next to flag and mapq in ONE word (no end column: 8 B per visit):
//   class 0 (span <= 256):   flag (16 bits) | mapq << 16 | (span - 1) << 24
//   class 1 (span <= 4096):  flag (12 bits) | mapq << 12 | (span - 1) << 20
// The SAM specification defines 12 flag bits; a read that sets a higher one (a uint16 can) and spans more
// than 256 bp goes to class 2, whose words hold all 16.
// A short read (span <= 256) whose (flag, mapq) pair has a code in the file's pair table, with 12-bit flags
// and pos inside its reference (the bucket index clamps positions to the reference; a packed word cannot
// carry a position the index does not vouch for), goes to the packed class instead: one word per read.
// codemap: 2^20 entries indexed by flag | mapq << 12, 0xFFFF = no code; NULL = no packed class.
__device__ __forceinline__ int read_class(int span, uint32_t flag, uint32_t mapq, int p, int64_t ref_bp,
                                          const uint16_t *__restrict__ codemap, uint32_t &code)
{
    if (span <= 256) {
        if (codemap && span >= 1 && flag < 4096u && p >= 0 && (int64_t)p < ref_bp) {
            code = codemap[flag | (mapq << 12)];
            if (code != 0xFFFFu) return BSIG_CLASS_PACKED;
        }
        return 0;
    }
    return (span <= 4096 && flag < 4096u) ? 1 : span <= 65536 ? 2 : 3;
}

// reference of read i: last r with ref_off[r] <= i
__device__ __forceinline__ int ref_of_read(const int64_t *__restrict__ ref_off, int n_ref, int64_t i)
{
    int lo = 0, hi = n_ref;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (ref_off[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

constexpr int kPrepThreads = 256;
constexpr int kPrepChunk = 2048;     // reads per workgroup in k_span_hist / k_scatter

// ---- the file's pair table: the (flag, mapq) pairs of short reads, counted on a sample --------------
// Any table is correct (a read whose pair has no code stays in class 0); a sample of the file finds the
// frequent pairs.  hist: 2^20 counters indexed by flag | mapq << 12.
__global__ __launch_bounds__(kPrepThreads) void k_pair_sample(int64_t n, int64_t chunk_stride,
                                                              const int32_t *__restrict__ pos, const int32_t *__restrict__ end,
                                                              const uint16_t *__restrict__ flag, const uint8_t *__restrict__ mapq,
                                                              uint32_t *__restrict__ hist)
{
    const int64_t base = (int64_t)blockIdx.x * chunk_stride * kPrepChunk;
    for (int r = 0; r < kPrepChunk / kPrepThreads; ++r) {
        const int64_t i = base + r * kPrepThreads + threadIdx.x;
        if (i >= n) break;
        const int span = end[i] - pos[i] + 1;
        const uint32_t f = flag[i];
        if (span >= 1 && span <= 256 && f < 4096u && pos[i] >= 0) atomicAdd(&hist[f | ((uint32_t)mapq[i] << 12)], 1u);
    }
}
// the non-empty counters as (key, count) pairs; *n_out may exceed cap (the caller then reads the counters themselves)
__global__ void k_pair_compact(const uint32_t *__restrict__ hist, uint32_t n_keys, uint2 *__restrict__ out, uint32_t cap,
                               uint32_t *__restrict__ n_out)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_keys) return;
    const uint32_t c = hist[k];
    if (!c) return;
    const uint32_t slot = atomicAdd(n_out, 1u);
    if (slot < cap) out[slot] = make_uint2(k, c);
}
// codemap[key of code c] = c (codemap was filled with 0xFFFF); fmtab[c] = flag | mapq << 16
__global__ void k_codemap_fill(const uint32_t *__restrict__ fmtab, int n_codes, uint16_t *__restrict__ codemap)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_codes) return;
    const uint32_t fm = fmtab[c];
    codemap[(fm & 0xFFFu) | ((fm >> 16) & 0xFFu) << 12] = (uint16_t)c;
}

// per-chunk class counts + per-class max span; also checks that the reads are sorted by position
// inside every reference (maxspan[BSIG_MAX_CLASSES] is set to 1 otherwise)
__global__ __launch_bounds__(kPrepThreads) void k_span_hist(int64_t n, int32_t n_ref,
                                                            const int64_t *__restrict__ ref_off,
                                                            const uint32_t *__restrict__ ref_units,
                                                            const int32_t *__restrict__ pos,
                                                            const int32_t *__restrict__ end,
                                                            const uint16_t *__restrict__ flag,
                                                            const uint8_t *__restrict__ mapq,
                                                            const uint16_t *__restrict__ codemap,
                                                            uint32_t *__restrict__ chunk_counts,
                                                            int32_t *__restrict__ maxspan)
{
    __shared__ uint32_t cnt[BSIG_MAX_CLASSES];
    __shared__ int32_t mx[BSIG_MAX_CLASSES];
    const int tid = threadIdx.x;
    if (tid < BSIG_MAX_CLASSES) { cnt[tid] = 0; mx[tid] = 0; }
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kPrepChunk;
    // per lane: how many of its reads fell into each class and their longest span; ONE LDS atomic per wave and class
    // at the end (an atomic per read had all 64 lanes of a wave queue up on one address: 1.6 of the kernel's 3.9 ms
    // on 5e8 reads)
    uint32_t my_cnt[BSIG_MAX_CLASSES];
    int32_t my_max[BSIG_MAX_CLASSES];
#pragma unroll
    for (int c = 0; c < BSIG_MAX_CLASSES; ++c) { my_cnt[c] = 0; my_max[c] = 0; }
    // (a chunk of 2,048 reads nearly always lies inside one reference: the search over the references' first reads,
    // four dependent loads per read, is made for the chunk's two ends -- uniform, scalar loads -- and per read only
    // where they differ)
    const int64_t last = (base + kPrepChunk < n ? base + kPrepChunk : n) - 1;
    const int rf_lo = ref_of_read(ref_off, n_ref, base < n ? base : n - 1), rf_hi = ref_of_read(ref_off, n_ref, last);
    for (int r = 0; r < kPrepChunk / kPrepThreads; ++r) {
        const int64_t i = base + r * kPrepThreads + tid;
        if (i < n) {
            const int p = pos[i];
            const int span = end[i] - p + 1;
            const int rf = rf_lo == rf_hi ? rf_lo : ref_of_read(ref_off, n_ref, i);
            uint32_t code;
            const int c = read_class(span, flag[i], mapq[i], p, (int64_t)ref_units[rf] << BSIG_REF_UNIT_SHIFT, codemap, code);
#pragma unroll
            for (int k = 0; k < BSIG_MAX_CLASSES; ++k) {
                my_cnt[k] += c == k ? 1u : 0u;
                my_max[k] = c == k && span > my_max[k] ? span : my_max[k];
            }
            // a position below its predecessor's is allowed only where a new reference starts
            if (i > 0 && p < pos[i - 1] && ref_off[rf] != i) maxspan[BSIG_MAX_CLASSES] = 1;
        }
    }
#pragma unroll
    for (int k = 0; k < BSIG_MAX_CLASSES; ++k) {
#pragma unroll
        for (int d = kWave / 2; d > 0; d >>= 1) {
            my_cnt[k] += __shfl_xor(my_cnt[k], d);
            const int32_t o = __shfl_xor(my_max[k], d);
            my_max[k] = o > my_max[k] ? o : my_max[k];
        }
        if ((tid & (kWave - 1)) == 0) {
            if (my_cnt[k]) atomicAdd(&cnt[k], my_cnt[k]);
            if (my_max[k] > 0) atomicMax(&mx[k], my_max[k]);
        }
    }
    __syncthreads();
    if (tid < BSIG_MAX_CLASSES) {
        chunk_counts[(int64_t)blockIdx.x * BSIG_MAX_CLASSES + tid] = cnt[tid];
        if (mx[tid] > 0) atomicMax(&maxspan[tid], mx[tid]);
    }
}

// The exclusive scan of the chunks' class counts (chunk_base[k][c] = reads of class c in the chunks before k) and the
// class totals, on the device: the counts used to travel to the host (4.9 MB for 5e8 reads), be summed there and come
// back as 9.8 MB of bases, 3 ms of every layout.  One workgroup: every thread sums a slab of consecutive chunks, the
// slab sums are scanned in LDS, every thread writes its slab's bases.
constexpr int kScanThreads = 1024;
__global__ __launch_bounds__(kScanThreads) void k_chunk_scan(int64_t n_chunks, const uint32_t *__restrict__ counts,
                                                             uint64_t *__restrict__ chunk_base, uint64_t *__restrict__ totals)
{
    __shared__ uint64_t slab[kScanThreads][BSIG_MAX_CLASSES];
    const int tid = threadIdx.x;
    const int64_t per = (n_chunks + kScanThreads - 1) / kScanThreads;
    const int64_t k0 = (int64_t)tid * per, k1 = k0 + per < n_chunks ? k0 + per : n_chunks;
    uint64_t sum[BSIG_MAX_CLASSES];
#pragma unroll
    for (int c = 0; c < BSIG_MAX_CLASSES; ++c) sum[c] = 0;
    for (int64_t k = k0; k < k1; ++k)
#pragma unroll
        for (int c = 0; c < BSIG_MAX_CLASSES; ++c) sum[c] += counts[k * BSIG_MAX_CLASSES + c];
#pragma unroll
    for (int c = 0; c < BSIG_MAX_CLASSES; ++c) slab[tid][c] = sum[c];
    __syncthreads();
    // inclusive scan over the slabs, in place (Hillis-Steele: ten steps)
    for (int d = 1; d < kScanThreads; d <<= 1) {
        uint64_t add[BSIG_MAX_CLASSES];
#pragma unroll
        for (int c = 0; c < BSIG_MAX_CLASSES; ++c) add[c] = tid >= d ? slab[tid - d][c] : 0;
        __syncthreads();
#pragma unroll
        for (int c = 0; c < BSIG_MAX_CLASSES; ++c) slab[tid][c] += add[c];
        __syncthreads();
    }
    uint64_t run[BSIG_MAX_CLASSES];
#pragma unroll
    for (int c = 0; c < BSIG_MAX_CLASSES; ++c) run[c] = slab[tid][c] - sum[c];
    for (int64_t k = k0; k < k1; ++k)
#pragma unroll
        for (int c = 0; c < BSIG_MAX_CLASSES; ++c) {
            chunk_base[k * BSIG_MAX_CLASSES + c] = run[c];
            run[c] += counts[k * BSIG_MAX_CLASSES + c];
        }
    if (tid == kScanThreads - 1)
#pragma unroll
        for (int c = 0; c < BSIG_MAX_CLASSES; ++c) totals[c] = slab[tid][c];
}

struct ScatterOut {
    int32_t *pos[BSIG_MAX_CLASSES];
    int32_t *end[BSIG_MAX_CLASSES];
    uint32_t *fm[BSIG_MAX_CLASSES];
    int32_t *tlen[BSIG_MAX_CLASSES];
    uint32_t *gb[BSIG_MAX_CLASSES];     // bucket number of every read (temporary)
    int32_t kshift[BSIG_MAX_CLASSES];
};

// stable partition of the reads into their classes; chunk_base = exclusive scan of chunk_counts
__global__ __launch_bounds__(kPrepThreads) void k_scatter(int64_t n, int32_t n_ref,
                                                          const int64_t *__restrict__ ref_off,
                                                          const uint32_t *__restrict__ ref_unit0,
                                                          const uint32_t *__restrict__ ref_units,
                                                          const int32_t *__restrict__ pos,
                                                          const int32_t *__restrict__ end,
                                                          const uint16_t *__restrict__ flag,
                                                          const uint8_t *__restrict__ mapq,
                                                          const int32_t *__restrict__ tlen,
                                                          const uint16_t *__restrict__ codemap,
                                                          const uint64_t *__restrict__ chunk_base,
                                                          const ScatterOut O)
{
    constexpr int NW = kPrepThreads / kWave;
    __shared__ uint32_t wcnt[NW][BSIG_MAX_CLASSES];
    __shared__ uint64_t run[BSIG_MAX_CLASSES];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
    if (tid < BSIG_MAX_CLASSES) run[tid] = chunk_base[(int64_t)blockIdx.x * BSIG_MAX_CLASSES + tid];
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kPrepChunk;
    // (the chunk's reference from its two ends, per read only where they differ: see k_span_hist)
    const int64_t last = (base + kPrepChunk < n ? base + kPrepChunk : n) - 1;
    const int rf_lo = ref_of_read(ref_off, n_ref, base < n ? base : n - 1), rf_hi = ref_of_read(ref_off, n_ref, last);
    for (int r = 0; r < kPrepChunk / kPrepThreads; ++r) {
        const int64_t i = base + r * kPrepThreads + tid;
        const bool valid = i < n;
        int p = 0, e = 0, cls = -1, rf = 0;
        uint32_t code = 0;
        if (valid) {
            p = pos[i]; e = end[i];
            rf = rf_lo == rf_hi ? rf_lo : ref_of_read(ref_off, n_ref, i);
            cls = read_class(e - p + 1, flag[i], mapq[i], p, (int64_t)ref_units[rf] << BSIG_REF_UNIT_SHIFT, codemap, code);
        }
        uint32_t rank = 0;
#pragma unroll
        for (int c = 0; c < BSIG_MAX_CLASSES; ++c) {
            const unsigned long long m = __ballot(cls == c);
            if (cls == c) rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (lane == 0) wcnt[wv][c] = (uint32_t)__popcll(m);
        }
        __syncthreads();
        if (valid) {
            uint64_t dst = run[cls] + rank;
            for (int k = 0; k < wv; ++k) dst += wcnt[k][cls];
            int64_t pp = p < 0 ? 0 : p;
            const int64_t ref_bp = (int64_t)ref_units[rf] << BSIG_REF_UNIT_SHIFT;
            if (pp >= ref_bp) pp = ref_bp - 1;
            const uint64_t g = ((uint64_t)ref_unit0[rf] << BSIG_REF_UNIT_SHIFT) + (uint64_t)pp;
            uint32_t fmw = (uint32_t)flag[i] | ((uint32_t)mapq[i] << 16);
            if (cls == BSIG_CLASS_PACKED) {
                fmw = ((uint32_t)p & kPackPosMask) | ((uint32_t)(e - p) << BSIG_PACK_POS_BITS) | (code << 23);   // span - 1 <= 255
            } else {
                O.pos[cls][dst] = p;
                if (cls == 0) fmw |= (uint32_t)(e - p) << 24;      // span - 1 <= 255
                else if (cls == 1) fmw = (uint32_t)flag[i] | ((uint32_t)mapq[i] << 12) | ((uint32_t)(e - p) << 20);   // flag < 4096, span - 1 <= 4095
                else O.end[cls][dst] = e;
            }
            O.fm[cls][dst] = fmw;
            O.tlen[cls][dst] = tlen[i];
            O.gb[cls][dst] = (uint32_t)(g >> O.kshift[cls]);
        }
        __syncthreads();
        if (tid < BSIG_MAX_CLASSES) {
            uint64_t t = 0;
            for (int k = 0; k < NW; ++k) t += wcnt[k][tid];
            run[tid] += t;
        }
        __syncthreads();
    }
}

// idx[b] = first read of the class with bucket >= b (gb is sorted)
__global__ void k_build_idx(int64_t n, const uint32_t *__restrict__ gb, uint64_t n_buckets,
                            uint32_t *__restrict__ idx)
{
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b > n_buckets) return;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((uint64_t)gb[mid] < b) lo = mid + 1; else hi = mid;
    }
    idx[b] = (uint32_t)lo;
}

// ------------------------------------------------------------------------------------------
// integrity of a resident layout that came from a reads file (bsig_reads_load)
// ------------------------------------------------------------------------------------------
// Order-independent 64-bit checksum of a run of 32-bit words: sum of mix(word, position).  Computed on the
// device where the data lies anyway (save: before the download; load: after the upload), so a reads file
// that rotted on disk is caught at HBM speed instead of a host CRC pass over 12 B per read.
__global__ __launch_bounds__(256) void k_checksum(const uint32_t *__restrict__ w, uint64_t n, uint64_t salt,
                                                  unsigned long long *__restrict__ acc)
{
    unsigned long long h = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        unsigned long long x = ((unsigned long long)w[i] << 32 | (uint32_t)(i * 0x9E3779B1ull)) ^ (i + salt) * 0xD6E8FEB86659FD93ull;
        x ^= x >> 32; x *= 0xD6E8FEB86659FD93ull; x ^= x >> 29;
        h += x;
    }
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) h += __shfl_xor(h, d);
    if ((threadIdx.x & (kWave - 1)) == 0 && h) atomicAdd(acc, h);
}

// a bucket index the pileup kernels may follow blindly: non-decreasing, ending at the class's read count
__global__ void k_check_idx(const uint32_t *__restrict__ idx, uint64_t n_buckets, uint32_t n_reads, int *__restrict__ bad)
{
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b > n_buckets) return;
    const uint32_t v = idx[b];
    if (v > n_reads || (b < n_buckets && v > idx[b + 1]) || (b == n_buckets && v != n_reads)) *bad = 1;
}

// ------------------------------------------------------------------------------------------
// read visits of a plan, for the roofline's algorithmic bytes:
//   acc[c], c = 0..3 = reads of span class c whose pos lies in the exact candidate window of
//                      their tile (SURVEY 8d's V, per class because class 0 reads are 4 B shorter)
//   acc[4]           = reads actually streamed (windows rounded to index buckets and to 4 reads)
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t lower_bound_pos(const int32_t *pos, uint32_t lo, uint32_t hi, int64_t key)
{
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)pos[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// the same over the packed words of one chunk (positions are base + the low bits' distance from base)
__device__ __forceinline__ uint32_t lower_bound_packed(const uint32_t *words, uint32_t lo, uint32_t hi, int64_t base, int64_t key)
{
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (base + (int64_t)((words[mid] - (uint32_t)base) & kPackPosMask) < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void k_visits(const BsigReadsDev R, const BsigKParams P, int mode,
                         const BsigWorkItem *__restrict__ items, int64_t n_items,
                         unsigned long long *__restrict__ acc)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_items) return;
    const BsigWorkItem w = items[t];
    int64_t tlo, thi;
    item_interval(w, P, mode, tlo, thi);
    unsigned long long streamed = 0;
    for (int c = 0; c < BSIG_SPAN_CLASSES; ++c) {
        const BsigClassCols &C = R.cls[c];
        if (C.n == 0) continue;
        uint32_t j_lo, j_hi;
        if (!class_window(C, w, tlo, thi, P.ext, j_lo, j_hi)) continue;
        streamed += ((j_hi + 3u) & ~3u) - (j_lo & ~3u);
        int64_t wlo = tlo - P.ext - C.maxspan + 1, whi = thi + P.ext;
        if (wlo < 0) wlo = 0;
        const uint32_t a = lower_bound_pos(C.pos, j_lo, j_hi, wlo);
        const uint32_t b = lower_bound_pos(C.pos, a, j_hi, whi);
        if (b > a) atomicAdd(&acc[c], (unsigned long long)(b - a));
    }
    {
        const BsigClassCols &C = R.cls[BSIG_CLASS_PACKED];
        int64_t rlo, rhi;
        if (packed_window(C, w, tlo, thi, P.ext, rlo, rhi)) {
            int64_t wlo = tlo - P.ext - C.maxspan + 1;
            const int64_t whi = thi + P.ext;
            if (wlo < 0) wlo = 0;
            const uint64_t g0 = (uint64_t)w.ref_unit0 << BSIG_REF_UNIT_SHIFT;
            unsigned long long v = 0;
            for (int64_t a = rlo; a < rhi; a += kPackChunk) {
                const int64_t b = a + kPackChunk < rhi ? a + kPackChunk : rhi;
                const uint32_t j_lo = C.idx[(g0 + (uint64_t)a) >> C.kshift], j_hi = C.idx[(g0 + (uint64_t)b) >> C.kshift];
                if (j_lo >= j_hi) continue;
                streamed += ((j_hi + 3u) & ~3u) - (j_lo & ~3u);
                const uint32_t x = lower_bound_packed(C.fm, j_lo, j_hi, a, wlo);
                const uint32_t y = lower_bound_packed(C.fm, x, j_hi, a, whi);
                v += y - x;
            }
            if (v) atomicAdd(&acc[BSIG_CLASS_PACKED], v);
        }
    }
    atomicAdd(&acc[BSIG_MAX_CLASSES], streamed);
}

}  // namespace

// ------------------------------------------------------------------------------------------
// launchers (called by runtime.hip)
// ------------------------------------------------------------------------------------------
namespace bsig {

// Tuning knobs (defaults from the environment once, changeable at run time through bsig_debug_set_knob for
// the sweep scripts): 0 = k_profile packed-class passes in flight (BAMSIGNALS_PROFILE_PRE), 1 = count tiles per
// wave (BAMSIGNALS_COUNT_TILES), 2 = count passes in flight (BAMSIGNALS_COUNT_PRE), 6 = k_profile_half's packed
// passes in flight (BAMSIGNALS_PROFILE_HALF_PRE).
static int g_knobs[7] = {-1, -1, -1, -1, -1, -1, -1};
static int knob(int k)
{
    static const char *const names[7] = {"BAMSIGNALS_PROFILE_PRE", "BAMSIGNALS_COUNT_TILES", "BAMSIGNALS_COUNT_PRE", "BAMSIGNALS_KNOB3",
                                         "BAMSIGNALS_KNOB4", "BAMSIGNALS_PROFILE_TILES", "BAMSIGNALS_PROFILE_HALF_PRE"};
    static const int dflt[7] = {2, 0, 0, 0, 0, 0, 2};
    if (g_knobs[k] < 0) {
        const char *e = getenv(names[k]);
        g_knobs[k] = e ? atoi(e) : dflt[k];
    }
    return g_knobs[k];
}

// The launch log (bsig_debug_launch_log, for the tests): the name of every pileup, overlap, sum-tiles and reduction-tiles
// (xcorr, frag, hist, summary, scaled, vplot, capped) kernel form launched while it is on -- the kernel template, its arguments and the
// run-time choices that change the code path.  The names are made in the dispatch macros below from the macros' own
// arguments, so a new branch reports itself; the occupancy query (tile_blocks_per_cu) shares the selectors and logs
// nothing.  Host code only; off, a launch pays one load and one branch.  Multi-slot calls launch from several threads: a
// mutex guards the text, which stops growing at 64 KB.
static std::atomic<int> g_log_on{0};
static std::mutex g_log_mu;
static std::string g_log_text;
static int g_log_names = 0;
static void log_launch(const char *fmt, ...)
{
    char name[160];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(name, sizeof name, fmt, ap);
    va_end(ap);
    std::lock_guard<std::mutex> lock(g_log_mu);
    if (g_log_text.size() + strlen(name) + 1 > (size_t)65536) return;
    g_log_text += name;
    g_log_text += '\n';
    ++g_log_names;
}
#define BSIG_LOG(...) do { if (__builtin_expect(g_log_on.load(std::memory_order_relaxed) != 0, 0)) log_launch(__VA_ARGS__); } while (0)

template <int NT>
static hipError_t launch_mode(int mode, int ss, const BsigReadsDev &R, const BsigKParams &P,
                              const BsigWorkItem *items, int64_t n_items, int tile_cells,
                              uint2 *windows, bool resolve_first, int32_t *out, hipStream_t st)
{
    if (n_items <= 0) return hipSuccess;
    // count family: consecutive tiles per wave and packed passes in flight (knobs 1 and 2, 0 = by the launch's size:
    // 8 x 4 from 65,536 tiles on -- eight tiles per wave still fill every SIMD eight times over --, 4 x 2 below;
    // scripts/count_sweep.py on config 3's tiling, final build: 1 x 4 0.139 ms, 2 x 2 0.122, 4 x 2 0.112, 8 x 4 0.107)
    const bool count_large = n_items >= 65536;
    const int count_tiles = knob(1) > 0 ? knob(1) : count_large ? 8 : 4, count_pre = knob(2) > 0 ? knob(2) : count_large ? 4 : 2;
    if (windows && resolve_first) {
        // P.resolved is set: the windows of every tile first (one lane per tile), with the lookup form of the parameters
        BsigKParams Q = P;
        Q.resolved = 0;
        hipLaunchKernelGGL(k_resolve_tiles, dim3((unsigned)((n_items + 255) / 256)), dim3(256), 0, st,
                           R, Q, mode, items, (uint32_t)n_items, reinterpret_cast<BsigResolved *>(windows));
    }
    const dim3 grid((unsigned)n_items), block(NT);
    if (mode == BSIG_MODE_PROFILE && tile_cells * (ss ? 2 : 1) <= kSmallCells && P.binsize > 1) {
        const int stride = (tile_cells * (ss ? 2 : 1)) | 1;
        const size_t lds = (size_t)((small_image_dwords(stride) + 3) & ~3) * sizeof(int32_t) + BSIG_PACK_CODES;   // + the packed class's table
        // (the form for resolved windows has no lookup code in it, as k_profile's)
#define BSIG_KS(SS_, RES_) do { BSIG_LOG("k_profile_small<%d,ss=%d,res=%d> acc=%d", NT, (int)SS_, (int)RES_, (int)P.accumulate); \
        hipLaunchKernelGGL((k_profile_small<NT, SS_, RES_>), grid, block, lds, st, items, (uint32_t)n_items, out, windows, R, P); } while (0)
        if (ss) { if (P.resolved) BSIG_KS(true, true); else BSIG_KS(true, false); }
        else    { if (P.resolved) BSIG_KS(false, true); else BSIG_KS(false, false); }
#undef BSIG_KS
    } else if (mode == BSIG_MODE_PROFILE) {
        // 16-bit counters + the packed class's table.  img_vec is ONE number in three places: it sizes the LDS here, and
        // k_profile / k_profile_half clear that many vectors and put the table right behind them (profile_tile takes it as
        // an argument; profile_multi_tiles computes the same from P.tile_cells, which is this tile_cells, and SS, which is ss)
        const uint32_t img_vec = (uint32_t)((tile_cells * (ss ? 2 : 1) + 8 + 7) / 8);
        const size_t lds = (size_t)img_vec * 16 + BSIG_PACK_CODES;
        // the packed class's passes requested before anything is consumed (knob 0: 2, 3 or 4; fewer = fewer VGPRs = more
        // resident waves, more = one round trip for denser windows)
        const int pre = knob(0);
        // the half form (P.packed_half: k_profile_half, k_profile_multi_half): one pass holds 8 * NT reads, a 2-kb tile's
        // ~410 at the north star's depth; knob 6 (BAMSIGNALS_PROFILE_HALF_PRE): passes requested up front, 1 or 2
        const bool half = P.packed_half != 0;
        const int pre_h = knob(6) <= 1 ? 1 : 2;
#define BSIG_KP(K_, SS_, PRE_, W_)                                                                                                      \
    do {                                                                                                                                \
        BSIG_LOG(#K_ "<%d,ss=%d,pre=%d,w=%d,res=%d> acc=%d", NT, (int)SS_, PRE_, W_, P.resolved ? 1 : 0, (int)P.accumulate);           \
        if (P.resolved) hipLaunchKernelGGL((K_<NT, SS_, PRE_, W_, true>), grid, block, lds, st, items, (uint32_t)n_items, img_vec, out, windows, R, P); \
        else hipLaunchKernelGGL((K_<NT, SS_, PRE_, W_, false>), grid, block, lds, st, items, (uint32_t)n_items, img_vec, out, windows, R, P); \
    } while (0)
#define BSIG_KPW(K_, SS_, PRE_) do { if (w8) BSIG_KP(K_, SS_, PRE_, 8); else BSIG_KP(K_, SS_, PRE_, 1); } while (0)
        // the build for 8 waves per SIMD (96 SGPRs, the rest kept in VGPR lanes; 57 VGPRs in the resolved form, which
        // alone has them to spare): narrow tiles -- many workgroups per byte moved -- gain from the eighth wave,
        // 2-kb tiles lose (same bases in 500 / 1,000 / 1,500 / 2,000-cell tiles, two launches, 7 -> 8 waves:
        // 354 -> 316, 227 -> 215, 212 -> 212, 187 -> 192 us).  knob 3: 8 = always, 1 = never, 0 = by the tile image
        const bool w8 = NT == kWave && P.resolved && (knob(3) == 8 || (knob(3) == 0 && lds <= 3072));
        // consecutive tiles per wave of a large launch (k_profile_multi).  One workgroup per tile, refilled by the
        // hardware as workgroups retire, is the better schedule down to 1-kb tiles (same bases, 7-8 waves, 1 / 2 / 4 tiles
        // per wave: 2-kb tiles 188 / 199 / 213 us, config 5's 1-kb tiles 145 / 155 / 166, config 4 398 / 420 / 431); for
        // 500-bp tiles four per wave win (317 / 299 / 282).  knob 5: 0 = four per wave for images of up to 2 KB
        // (about 760 cells), 1 = never, 2 / 4 = always
        const int pt = knob(5) == 0 ? (lds <= 2048 ? 4 : 1) : knob(5);
        if (NT == kWave && P.resolved && !P.accumulate && pt > 1) {
            const int T = pt >= 4 ? 4 : 2;
            const dim3 g2((unsigned)((n_items + T - 1) / T));
            const size_t lds_m = lds + (size_t)T * 20 * sizeof(uint32_t);
#define BSIG_KM(K_, SS_, PRE_, W_, T_) do { BSIG_LOG(#K_ "<ss=%d,pre=%d,w=%d,T=%d> acc=%d", (int)SS_, PRE_, W_, T_, (int)P.accumulate); \
        hipLaunchKernelGGL((K_<SS_, PRE_, W_, T_>), g2, dim3(kWave), lds_m, st, items, (uint32_t)n_items, out, windows, R, P); } while (0)
#define BSIG_KMT(K_, SS_, PRE_, W_) do { if (T == 4) BSIG_KM(K_, SS_, PRE_, W_, 4); else BSIG_KM(K_, SS_, PRE_, W_, 2); } while (0)
#define BSIG_KMW(K_, SS_, PRE_) do { if (w8) BSIG_KMT(K_, SS_, PRE_, 8); else BSIG_KMT(K_, SS_, PRE_, 1); } while (0)
            if (half) {
                if (ss) { if (pre_h == 1) BSIG_KMW(k_profile_multi_half, true, 1); else BSIG_KMW(k_profile_multi_half, true, 2); }
                else    { if (pre_h == 1) BSIG_KMW(k_profile_multi_half, false, 1); else BSIG_KMW(k_profile_multi_half, false, 2); }
            } else {
                if (ss) BSIG_KMW(k_profile_multi, true, 2);
                else    BSIG_KMW(k_profile_multi, false, 2);
            }
#undef BSIG_KMW
#undef BSIG_KMT
#undef BSIG_KM
            return hipGetLastError();
        }
        if (half) {
            if (ss) { if (pre_h == 1) BSIG_KPW(k_profile_half, true, 1); else BSIG_KPW(k_profile_half, true, 2); }
            else    { if (pre_h == 1) BSIG_KPW(k_profile_half, false, 1); else BSIG_KPW(k_profile_half, false, 2); }
            return hipGetLastError();
        }
        if (ss) { if (pre <= 2) BSIG_KPW(k_profile, true, 2); else if (pre == 3) BSIG_KP(k_profile, true, 3, 1); else BSIG_KP(k_profile, true, 4, 1); }
        else    { if (pre <= 2) BSIG_KPW(k_profile, false, 2); else if (pre == 3) BSIG_KP(k_profile, false, 3, 1); else BSIG_KP(k_profile, false, 4, 1); }
#undef BSIG_KPW
#undef BSIG_KP
    } else if (mode == BSIG_MODE_COVERAGE && (P.binsize > 1 || ss)) {
        // bins and / or strands (k_coverage_bins): int32 difference image, the scan totals, the packed class's table
        const int S = ss ? 2 : 1;
        BsigKParams Q = P;
        Q.cov_reps = cov_bins_reps(tile_cells * S);
        const size_t lds = (size_t)cov_bins_vec(tile_cells * S) * Q.cov_reps * 16 + (size_t)((S * NT / 64 + 3) / 4) * 16 + BSIG_PACK_CODES;
        // (a resized plan, P.frag_len != 0, has instantiations of its own -- covered_interval says why -- and names them)
#define BSIG_KB(RES_, SS_) do { if (P.frag_len) { \
            BSIG_LOG("k_coverage_bins<%d,pre=2,res=%d,ss=%d,frag=1> acc=%d cov_reps=%d", NT, (int)RES_, (int)SS_, (int)Q.accumulate, (int)Q.cov_reps); \
            hipLaunchKernelGGL((k_coverage_bins<NT, 2, RES_, SS_, true>), grid, block, lds, st, items, (uint32_t)n_items, out, windows, R, Q); \
        } else { \
            BSIG_LOG("k_coverage_bins<%d,pre=2,res=%d,ss=%d> acc=%d cov_reps=%d", NT, (int)RES_, (int)SS_, (int)Q.accumulate, (int)Q.cov_reps); \
            hipLaunchKernelGGL((k_coverage_bins<NT, 2, RES_, SS_>), grid, block, lds, st, items, (uint32_t)n_items, out, windows, R, Q); } } while (0)
        if (ss) { if (P.resolved) BSIG_KB(true, true); else BSIG_KB(false, true); }
        else    { if (P.resolved) BSIG_KB(true, false); else BSIG_KB(false, false); }
#undef BSIG_KB
    } else if (mode == BSIG_MODE_COVERAGE) {
        const size_t lds = (size_t)((tile_cells + 8 + 7) / 8) * 16 + (size_t)((NT / 64 + 3) / 4) * 16 + BSIG_PACK_CODES;   // signed 16-bit cells, scan totals, the packed class's table
        // (the packed class's passes hold 256 reads each: two in flight cover a 2-kb tile at 100-fold coverage; the form
        // for resolved windows has no lookup code in it)
        if (P.frag_len) {
            BSIG_LOG("k_coverage<%d,pre=2,res=%d,frag=1> acc=%d", NT, P.resolved ? 1 : 0, (int)P.accumulate);
            if (P.resolved) hipLaunchKernelGGL((k_coverage<NT, 2, true, true>), grid, block, lds, st, items, (uint32_t)n_items, out, windows, R, P);
            else hipLaunchKernelGGL((k_coverage<NT, 2, false, true>), grid, block, lds, st, items, (uint32_t)n_items, out, windows, R, P);
            return hipGetLastError();
        }
        BSIG_LOG("k_coverage<%d,pre=2,res=%d> acc=%d", NT, P.resolved ? 1 : 0, (int)P.accumulate);
        if (P.resolved) hipLaunchKernelGGL((k_coverage<NT, 2, true>), grid, block, lds, st, items, (uint32_t)n_items, out, windows, R, P);
        else hipLaunchKernelGGL((k_coverage<NT, 2, false>), grid, block, lds, st, items, (uint32_t)n_items, out, windows, R, P);
    } else if (P.minoverlap > 0 && NT == kWave && (!windows || P.resolved) && count_tiles > 1) {
        // bamOverlaps (a count plan never comes here: its minoverlap is 0), several tiles per wave as below, in fewer
        // forms than the count family has: knob 1 (tiles per wave) 2 .. 7 -> 4, 8 and more -> 8 (1: the one-tile kernel);
        // knob 2 (passes up front) up to 2 -> 2, 3 and more -> 4
        const int T = count_tiles >= 8 ? 8 : 4;
        const dim3 g2((unsigned)((n_items + T - 1) / T));
#define BSIG_OM(T_, PRE_, W_) do { BSIG_LOG("k_overlap_multi<T=%d,pre=%d,within=%d> acc=%d", T_, PRE_, (int)W_, (int)P.accumulate); \
        hipLaunchKernelGGL((k_overlap_multi<T_, PRE_, W_>), g2, dim3(kWave), 0, st, items, (uint32_t)n_items, out, windows, R, P); } while (0)
#define BSIG_OMW(T_, PRE_) do { if (P.within) BSIG_OM(T_, PRE_, true); else BSIG_OM(T_, PRE_, false); } while (0)
        if (count_pre <= 2) { if (T == 8) BSIG_OMW(8, 2); else BSIG_OMW(4, 2); }
        else                { if (T == 8) BSIG_OMW(8, 4); else BSIG_OMW(4, 4); }
#undef BSIG_OMW
#undef BSIG_OM
    } else if (P.minoverlap > 0) {
        BSIG_LOG("k_overlap<%d,within=%d> acc=%d", NT, P.within ? 1 : 0, (int)P.accumulate);
        if (P.within) hipLaunchKernelGGL((k_overlap<NT, true>), grid, block, 0, st, items, (uint32_t)n_items, out, windows, R, P);
        else hipLaunchKernelGGL((k_overlap<NT, false>), grid, block, 0, st, items, (uint32_t)n_items, out, windows, R, P);
    } else if (NT == kWave && (!windows || P.resolved) && count_tiles > 1) {
        // several consecutive tiles per wave (the slices of heavy tiles, which come with fixed windows, and
        // the wider workgroups keep the one-tile kernel)
        const int T = count_tiles >= 8 ? 8 : count_tiles >= 4 ? 4 : 2;
        const dim3 g2((unsigned)((n_items + T - 1) / T));
#define BSIG_CM(T_, PRE_) do { BSIG_LOG("k_count_multi<T=%d,pre=%d> acc=%d", T_, PRE_, (int)P.accumulate); \
        hipLaunchKernelGGL((k_count_multi<T_, PRE_>), g2, dim3(kWave), 0, st, items, (uint32_t)n_items, out, windows, R, P); } while (0)
        if (count_pre <= 2)      { if (T == 8) BSIG_CM(8, 2); else if (T == 4) BSIG_CM(4, 2); else BSIG_CM(2, 2); }
        else if (count_pre == 3) { if (T == 8) BSIG_CM(8, 3); else if (T == 4) BSIG_CM(4, 3); else BSIG_CM(2, 3); }
        else                     { if (T == 8) BSIG_CM(8, 4); else if (T == 4) BSIG_CM(4, 4); else BSIG_CM(2, 4); }
#undef BSIG_CM
    } else {
        BSIG_LOG("k_count<%d> acc=%d", NT, (int)P.accumulate);
        hipLaunchKernelGGL((k_count<NT>), grid, block, 0, st, items, (uint32_t)n_items, out, windows, R, P);
    }
    return hipGetLastError();
}

hipError_t launch_pileup(int mode, int ss, int threads, const BsigReadsDev &R, const BsigKParams &P,
                         const BsigWorkItem *items, int64_t n_items, int tile_cells,
                         void *windows, bool resolve_first, int32_t *out, hipStream_t st)
{
    switch (threads) {
    case 64:  return launch_mode<64>(mode, ss, R, P, items, n_items, tile_cells, (uint2 *)windows, resolve_first, out, st);
    case 128: return launch_mode<128>(mode, ss, R, P, items, n_items, tile_cells, (uint2 *)windows, resolve_first, out, st);
    case 256: return launch_mode<256>(mode, ss, R, P, items, n_items, tile_cells, (uint2 *)windows, resolve_first, out, st);
    default:  return hipErrorInvalidValue;
    }
}

// ---- a tile-kernel form (kernels.h): every reduction kind below has a selector from its run-time choices to one --------
// The parameters every tile kernel begins with.  A selector's `f` takes the kernel by its full type, the kind's own
// parameters after these, so an instantiation that expects other arguments than the kind's launch passes does not compile.
#define BSIG_TILE_PARAMS(Out_) const BsigWorkItem *, const uint2 *, Out_ *, const uint2 *, BsigReadsDev, BsigKParams

int tile_blocks_per_cu(const TileForm &f)
{
    int nb = 0;
    const hipError_t e = f.kernel ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, f.kernel, f.threads, f.lds) : hipErrorInvalidValue;
    return e == hipSuccess && nb > 0 ? nb : 1;
}

// One workgroup of form f per run.  extra: the kernel's arguments after (items, runs, out, windows, R, P), of exactly its
// parameter types.  windows && resolve_first: P.resolved is set, and the windows of every tile are looked up first (one
// lane per tile), with the lookup form of the parameters.
template <typename... Extra>
static hipError_t launch_tiles(const TileForm &f, const BsigReadsDev &R, const BsigKParams &P, const BsigWorkItem *items, int64_t n_items,
                               const uint2 *runs, int64_t n_runs, void *windows, bool resolve_first, void *out, hipStream_t st,
                               Extra... extra)
{
    if (n_runs <= 0) return hipSuccess;
    if (!f.kernel) return hipErrorInvalidValue;
    if (windows && resolve_first) {
        BsigKParams Q = P;
        Q.resolved = 0;
        hipLaunchKernelGGL(k_resolve_tiles, dim3((unsigned)((n_items + 255) / 256)), dim3(256), 0, st,
                           R, Q, f.mode, items, (uint32_t)n_items, reinterpret_cast<BsigResolved *>(windows));
    }
    BSIG_LOG("%s", f.name);
    void *args[] = {&items, &runs, &out, &windows, const_cast<BsigReadsDev *>(&R), const_cast<BsigKParams *>(&P), &extra...};
    const hipError_t e = hipLaunchKernel(f.kernel, dim3((unsigned)n_runs), dim3((unsigned)f.threads), args, f.lds, st);
    const hipError_t last = hipGetLastError();      // (the lookup launch's, if that failed)
    return e != hipSuccess ? e : last;
}

// ---- sums over ranges -------------------------------------------------------------------------------------------
static size_t sum_tiles_lds(int kind, int ss, int nw, int tile_cells)
{
    const int vals = tile_cells * (ss ? 2 : 1);
    const int acc_v = (vals + 3) / 4, img_v = kind == kSumCoverSS ? (vals + 3) / 4 : (vals + 7) / 8;
    return (size_t)(acc_v + img_v * nw) * 16 + BSIG_PACK_CODES;
}

// one k_sum_tiles instantiation by its run-time choices (frag: the coverage kinds of a resized plan)
TileForm sum_form(int kind, int ss, int nw, bool half, bool res, bool frag, int tile_cells)
{
    const auto f = [&](void (*k)(BSIG_TILE_PARAMS(int32_t)), const char *name) {
        return TileForm{reinterpret_cast<const void *>(k), name, nw * kWave, sum_tiles_lds(kind, ss, nw, tile_cells),
                        kind == kSumProfile ? BSIG_MODE_PROFILE : BSIG_MODE_COVERAGE};
    };
#define BSIG_SK(NW_, K_, SS_, H_) do { if (res) return f(k_sum_tiles<NW_, K_, (SS_) != 0, (H_) != 0, true>, "k_sum_tiles<nw=" #NW_ "," #K_ ",ss=" #SS_ ",half=" #H_ ",res=1>"); \
                                        else return f(k_sum_tiles<NW_, K_, (SS_) != 0, (H_) != 0, false>, "k_sum_tiles<nw=" #NW_ "," #K_ ",ss=" #SS_ ",half=" #H_ ",res=0>"); } while (0)
// (the coverage kinds of a resized plan: instantiations of their own, see covered_interval)
#define BSIG_SKF(NW_, K_, SS_) do { if (res) return f(k_sum_tiles<NW_, K_, (SS_) != 0, false, true, true>, "k_sum_tiles<nw=" #NW_ "," #K_ ",ss=" #SS_ ",half=0,res=1,frag=1>"); \
                                     else return f(k_sum_tiles<NW_, K_, (SS_) != 0, false, false, true>, "k_sum_tiles<nw=" #NW_ "," #K_ ",ss=" #SS_ ",half=0,res=0,frag=1>"); } while (0)
#define BSIG_SKFN(K_, SS_) do { if (nw == 1) BSIG_SKF(1, K_, SS_); else if (nw == 2) BSIG_SKF(2, K_, SS_); else BSIG_SKF(4, K_, SS_); } while (0)
#define BSIG_SKN(K_, SS_, H_) do { if (nw == 1) BSIG_SK(1, K_, SS_, H_); else if (nw == 2) BSIG_SK(2, K_, SS_, H_); else BSIG_SK(4, K_, SS_, H_); } while (0)
    if (nw != 1 && nw != 2 && nw != 4) return TileForm{};
    if (kind == kSumProfile) {
        if (ss) { if (half) BSIG_SKN(kSumProfile, 1, 1); else BSIG_SKN(kSumProfile, 1, 0); }
        else    { if (half) BSIG_SKN(kSumProfile, 0, 1); else BSIG_SKN(kSumProfile, 0, 0); }
    } else if (kind == kSumCover) {
        if (frag) BSIG_SKFN(kSumCover, 0); else BSIG_SKN(kSumCover, 0, 0);
    } else if (kind == kSumCoverSS) {
        if (frag) BSIG_SKFN(kSumCoverSS, 1); else BSIG_SKN(kSumCoverSS, 1, 0);
    }
#undef BSIG_SKFN
#undef BSIG_SKF
#undef BSIG_SKN
#undef BSIG_SK
    return TileForm{};
}

hipError_t launch_sum_tiles(int kind, int ss, int nw, const BsigReadsDev &R, const BsigKParams &P, const BsigWorkItem *items,
                            int64_t n_items, const uint2 *runs, int64_t n_runs, void *windows, bool resolve_first, int32_t *slab,
                            hipStream_t st)
{
    return launch_tiles(sum_form(kind, ss, nw, P.packed_half != 0, P.resolved != 0, P.frag_len != 0, P.tile_cells), R, P, items, n_items,
                        runs, n_runs, windows, resolve_first, slab, st);
}

hipError_t launch_sum_reduce(bool is_signed, const int32_t *slab, int32_t slab_vals, const BsigSumChunk *chunks, int64_t n_chunks,
                             int32_t max_nvals, unsigned long long *base, hipStream_t st)
{
    if (n_chunks <= 0) return hipSuccess;
    const dim3 grid((unsigned)((max_nvals + 1023) / 1024), (unsigned)n_chunks);
    if (is_signed) hipLaunchKernelGGL(k_sum_reduce<true>, grid, dim3(256), 0, st, slab, slab_vals, chunks, base);
    else hipLaunchKernelGGL(k_sum_reduce<false>, grid, dim3(256), 0, st, slab, slab_vals, chunks, base);
    return hipGetLastError();
}

hipError_t launch_sum_scan(long long *base, int32_t width, int32_t tile_cells, int32_t S, hipStream_t st)
{
    if (width <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_sum_scan, dim3((unsigned)((width + tile_cells - 1) / tile_cells), (unsigned)S), dim3(256), 0, st,
                       base, width, tile_cells, S);
    return hipGetLastError();
}

hipError_t launch_sum_bins(const long long *base, int32_t width, int32_t binsize, int32_t S, int64_t n_out, long long *out, hipStream_t st)
{
    if (n_out <= 0) return hipSuccess;
    if (binsize > 64) hipLaunchKernelGGL(k_sum_bins<true>, dim3((unsigned)((n_out + 3) / 4)), dim3(256), 0, st, base, width, binsize, S, n_out, out);
    else hipLaunchKernelGGL(k_sum_bins<false>, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, st, base, width, binsize, S, n_out, out);
    return hipGetLastError();
}

// ---- strand cross-correlation --------------------------------------------------------------------------------------
static size_t xcorr_tiles_lds(bool wide, int tile_cells, int body, int max_lag)
{
    return (size_t)xcorr_lds(wide, tile_cells, body, max_lag).total * 4;
}

// one k_xcorr_tiles instantiation by its run-time choices
TileForm xcorr_form(int threads, bool half, bool wide, int tile_cells, int body, int max_lag)
{
    const auto f = [&](void (*k)(BSIG_TILE_PARAMS(unsigned long long), int, int, unsigned long long), const char *name) {
        return TileForm{reinterpret_cast<const void *>(k), name, threads, xcorr_tiles_lds(wide, tile_cells, body, max_lag), BSIG_MODE_PROFILE};
    };
#define BSIG_XK(NT_) do { if (wide) return f(k_xcorr_tiles<NT_, false, true>, "k_xcorr_tiles<" #NT_ ",half=0,wide=1>"); \
                          if (half) return f(k_xcorr_tiles<NT_, true, false>, "k_xcorr_tiles<" #NT_ ",half=1,wide=0>"); \
                          return f(k_xcorr_tiles<NT_, false, false>, "k_xcorr_tiles<" #NT_ ",half=0,wide=0>"); } while (0)
    if (threads == 64) BSIG_XK(64);
    if (threads == 128) BSIG_XK(128);
    if (threads == 256) BSIG_XK(256);
#undef BSIG_XK
    return TileForm{};
}

hipError_t launch_xcorr_tiles(int threads, bool wide, const BsigReadsDev &R, const BsigKParams &P, const BsigWorkItem *items,
                              int64_t n_items, const uint2 *runs, int64_t n_runs, void *windows, bool resolve_first, int body,
                              int max_lag, unsigned long long n_cells, unsigned long long *out, hipStream_t st)
{
    return launch_tiles(xcorr_form(threads, !wide && P.packed_half != 0, wide, P.tile_cells, body, max_lag), R, P, items, n_items, runs,
                        n_runs, windows, resolve_first, out, st, body, max_lag, n_cells);
}

// ---- fragment-length histogram --------------------------------------------------------------------------------------
static bool frag_ltab(int n_rows) { return (size_t)frag_hist_dwords(n_rows) * 4 + BSIG_PACK_CODES <= 65536; }
static size_t frag_tiles_lds(int n_rows)
{
    return (size_t)frag_hist_dwords(n_rows) * 4 + (frag_ltab(n_rows) ? BSIG_PACK_CODES : 0);
}

// one k_frag_tiles instantiation by its run-time choices (ltab: by n_rows, whether the filter table fits beside the rows)
TileForm frag_form(int threads, bool merge, int n_rows)
{
    const bool ltab = frag_ltab(n_rows);
    const auto f = [&](void (*k)(BSIG_TILE_PARAMS(unsigned long long), int, int), const char *name) {
        return TileForm{reinterpret_cast<const void *>(k), name, threads, frag_tiles_lds(n_rows), BSIG_MODE_COUNT};
    };
#define BSIG_FK(NT_) do { if (merge) { if (ltab) return f(k_frag_tiles<NT_, true, true>, "k_frag_tiles<" #NT_ ",merge=1,ltab=1>"); \
                                       return f(k_frag_tiles<NT_, true, false>, "k_frag_tiles<" #NT_ ",merge=1,ltab=0>"); } \
                          if (ltab) return f(k_frag_tiles<NT_, false, true>, "k_frag_tiles<" #NT_ ",merge=0,ltab=1>"); \
                          return f(k_frag_tiles<NT_, false, false>, "k_frag_tiles<" #NT_ ",merge=0,ltab=0>"); } while (0)
    if (threads == 64) BSIG_FK(64);
    if (threads == 128) BSIG_FK(128);
    if (threads == 256) BSIG_FK(256);
#undef BSIG_FK
    return TileForm{};
}

hipError_t launch_frag_tiles(int threads, bool merge, const BsigReadsDev &R, const BsigKParams &P, const BsigWorkItem *items,
                             int64_t n_items, const uint2 *runs, int64_t n_runs, void *windows, bool resolve_first, int n_rows,
                             int lenbin, unsigned long long *out, hipStream_t st)
{
    return launch_tiles(frag_form(threads, merge, n_rows), R, P, items, n_items, runs, n_runs, windows, resolve_first, out, st, n_rows,
                        lenbin);
}

// ---- V-plot -------------------------------------------------------------------------------------------------------------
// (ltab: the global form keeps nothing else in LDS; the LDS form by whether the filter table fits the budget behind the table)
static bool vplot_ltab(bool global, int n_cells, size_t lds_budget)
{
    return (size_t)vplot_tab_dwords(global, n_cells) * 4 + BSIG_PACK_CODES <= lds_budget;
}

// one k_vplot_tiles instantiation by its run-time choices
TileForm vplot_form(int threads, bool global, bool merge, int n_cells, size_t lds_budget)
{
    const bool ltab = vplot_ltab(global, n_cells, lds_budget);
    const auto f = [&](void (*k)(BSIG_TILE_PARAMS(unsigned long long), int, int, int, int, uint32_t, int), const char *name) {
        return TileForm{reinterpret_cast<const void *>(k), name, threads,
                        (size_t)vplot_tab_dwords(global, n_cells) * 4 + (ltab ? BSIG_PACK_CODES : 0), BSIG_MODE_COUNT};
    };
#define BSIG_VKM(NT_, M_) do { if (global) return f(k_vplot_tiles<NT_, true, true, (M_) != 0>, "k_vplot_tiles<" #NT_ ",global=1,ltab=1,merge=" #M_ ">"); \
                               if (ltab) return f(k_vplot_tiles<NT_, false, true, (M_) != 0>, "k_vplot_tiles<" #NT_ ",global=0,ltab=1,merge=" #M_ ">"); \
                               return f(k_vplot_tiles<NT_, false, false, (M_) != 0>, "k_vplot_tiles<" #NT_ ",global=0,ltab=0,merge=" #M_ ">"); } while (0)
#define BSIG_VK(NT_) do { if (merge) BSIG_VKM(NT_, 1); else BSIG_VKM(NT_, 0); } while (0)
    if (threads == 64) BSIG_VK(64);
    if (threads == 128) BSIG_VK(128);
    if (threads == 256) BSIG_VK(256);
#undef BSIG_VK
#undef BSIG_VKM
    return TileForm{};
}

hipError_t launch_vplot_tiles(int threads, bool global, bool merge, size_t lds_budget, const BsigReadsDev &R, const BsigKParams &P,
                              const BsigWorkItem *items, int64_t n_items, const uint2 *runs, int64_t n_runs, void *windows,
                              bool resolve_first, int n_rows, int n_cols, int lenbin, int binsize, uint32_t bin_magic, int bin_shift,
                              unsigned long long *out, hipStream_t st)
{
    return launch_tiles(vplot_form(threads, global, merge, n_rows * n_cols, lds_budget), R, P, items, n_items, runs, n_runs, windows,
                        resolve_first, out, st, n_rows, n_cols, lenbin, binsize, bin_magic, bin_shift);
}

// ---- depth histogram -----------------------------------------------------------------------------------------------
static size_t hist_tiles_lds(bool coverage, bool wide, int tile_cells, int n_rows)
{
    return (size_t)hist_lds(coverage ? kHistCover : kHistEnds, wide, tile_cells, n_rows).total * 4;
}

// one k_hist_tiles instantiation by its run-time choices
TileForm hist_form(int threads, bool coverage, bool half, bool wide, bool merge, int tile_cells, int n_rows)
{
    const auto f = [&](void (*k)(BSIG_TILE_PARAMS(unsigned long long), int, unsigned long long), const char *name) {
        return TileForm{reinterpret_cast<const void *>(k), name, threads, hist_tiles_lds(coverage, wide, tile_cells, n_rows),
                        coverage ? BSIG_MODE_COVERAGE : BSIG_MODE_PROFILE};
    };
#define BSIG_HN(NT_, K_, W_, F_) f(k_hist_tiles<NT_, K_, (W_) != 0, F_>, "k_hist_tiles<" #NT_ "," #K_ ",wide=" #W_ ",form=" #F_ ">")
#define BSIG_HF(NT_, F_) do { if (coverage) { if (wide) return BSIG_HN(NT_, kHistCover, 1, F_); return BSIG_HN(NT_, kHistCover, 0, F_); } \
                              if (wide) return BSIG_HN(NT_, kHistEnds, 1, F_); \
                              if (half) return BSIG_HN(NT_, kHistEndsHalf, 0, F_); \
                              return BSIG_HN(NT_, kHistEnds, 0, F_); } while (0)
#define BSIG_HK(NT_) do { if (merge) BSIG_HF(NT_, 1); BSIG_HF(NT_, 0); } while (0)
    if (threads == 64) BSIG_HK(64);
    if (threads == 128) BSIG_HK(128);
    if (threads == 256) BSIG_HK(256);
#undef BSIG_HK
#undef BSIG_HF
#undef BSIG_HN
    return TileForm{};
}

hipError_t launch_hist_tiles(int threads, bool coverage, bool wide, bool merge, const BsigReadsDev &R, const BsigKParams &P,
                             const BsigWorkItem *items, int64_t n_items, const uint2 *runs, int64_t n_runs, void *windows,
                             bool resolve_first, int n_rows, unsigned long long n_cells, unsigned long long *out, hipStream_t st)
{
    return launch_tiles(hist_form(threads, coverage, !wide && P.packed_half != 0, wide, merge, P.tile_cells, n_rows), R, P, items, n_items,
                        runs, n_runs, windows, resolve_first, out, st, n_rows, n_cells);
}

// ---- per-range summaries -------------------------------------------------------------------------------------------
static size_t summary_tiles_lds(bool coverage, bool wide, int tile_cells)
{
    return (size_t)summary_lds(coverage ? kHistCover : kHistEnds, wide, tile_cells).total * 4;
}

// one k_summary_tiles instantiation by its run-time choices
TileForm summary_form(int threads, bool coverage, bool half, bool wide, int tile_cells)
{
    const auto f = [&](void (*k)(BSIG_TILE_PARAMS(unsigned long long), BsigThresholds), const char *name) {
        return TileForm{reinterpret_cast<const void *>(k), name, threads, summary_tiles_lds(coverage, wide, tile_cells),
                        coverage ? BSIG_MODE_COVERAGE : BSIG_MODE_PROFILE};
    };
#define BSIG_SN(NT_, K_, W_) f(k_summary_tiles<NT_, K_, (W_) != 0>, "k_summary_tiles<" #NT_ "," #K_ ",wide=" #W_ ">")
#define BSIG_SK(NT_) do { if (coverage) { if (wide) return BSIG_SN(NT_, kHistCover, 1); return BSIG_SN(NT_, kHistCover, 0); } \
                          if (wide) return BSIG_SN(NT_, kHistEnds, 1); \
                          if (half) return BSIG_SN(NT_, kHistEndsHalf, 0); \
                          return BSIG_SN(NT_, kHistEnds, 0); } while (0)
    if (threads == 64) BSIG_SK(64);
    if (threads == 128) BSIG_SK(128);
    if (threads == 256) BSIG_SK(256);
#undef BSIG_SK
#undef BSIG_SN
    return TileForm{};
}

hipError_t launch_summary_tiles(int threads, bool coverage, bool wide, const BsigReadsDev &R, const BsigKParams &P,
                                const BsigWorkItem *items, int64_t n_items, const uint2 *runs, int64_t n_runs, void *windows,
                                bool resolve_first, const BsigThresholds &T, unsigned long long *out, hipStream_t st)
{
    return launch_tiles(summary_form(threads, coverage, !wide && P.packed_half != 0, wide, P.tile_cells), R, P, items, n_items, runs,
                        n_runs, windows, resolve_first, out, st, T);
}

hipError_t launch_summary_finish(int64_t n_rows, int stride, long long *out, hipStream_t st)
{
    if (n_rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_summary_finish, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, st, out, (long long)n_rows, stride);
    return hipGetLastError();
}

// ---- scaled regions ------------------------------------------------------------------------------------------------
static size_t scaled_tiles_lds(bool coverage, bool wide, int tile_cells, int rows, int n_bins)
{
    return (size_t)scaled_lds(coverage ? kHistCover : kHistEnds, wide, tile_cells, rows, n_bins).total * 4;
}

// one k_scaled_tiles instantiation by its run-time choices (rows: 2 for 5' ends with strands, else 1)
TileForm scaled_form(int threads, bool coverage, bool half, bool wide, bool seg, int tile_cells, int rows, int n_bins)
{
    const auto f = [&](void (*k)(BSIG_TILE_PARAMS(unsigned long long), int), const char *name) {
        return TileForm{reinterpret_cast<const void *>(k), name, threads, scaled_tiles_lds(coverage, wide, tile_cells, rows, n_bins),
                        coverage ? BSIG_MODE_COVERAGE : BSIG_MODE_PROFILE};
    };
#define BSIG_SN(NT_, K_, W_, S_) f(k_scaled_tiles<NT_, K_, (W_) != 0, (S_) != 0>, "k_scaled_tiles<" #NT_ "," #K_ ",wide=" #W_ ",seg=" #S_ ">")
#define BSIG_SC(NT_) do { if (coverage) { if (wide) return BSIG_SN(NT_, kHistCover, 1, 0); \
                                          if (seg) return BSIG_SN(NT_, kHistCover, 0, 1); \
                                          return BSIG_SN(NT_, kHistCover, 0, 0); } \
                          if (wide) return BSIG_SN(NT_, kHistEnds, 1, 0); \
                          if (half) { if (seg) return BSIG_SN(NT_, kHistEndsHalf, 0, 1); \
                                      return BSIG_SN(NT_, kHistEndsHalf, 0, 0); } \
                          if (seg) return BSIG_SN(NT_, kHistEnds, 0, 1); \
                          return BSIG_SN(NT_, kHistEnds, 0, 0); } while (0)
    if (threads == 64) BSIG_SC(64);
    if (threads == 128) BSIG_SC(128);
    if (threads == 256) BSIG_SC(256);
#undef BSIG_SC
#undef BSIG_SN
    return TileForm{};
}

hipError_t launch_scaled_tiles(int threads, bool coverage, bool wide, bool segmented, const BsigReadsDev &R, const BsigKParams &P,
                               const BsigWorkItem *items, int64_t n_items, const uint2 *runs, int64_t n_runs, void *windows,
                               bool resolve_first, int n_bins, unsigned long long *out, hipStream_t st)
{
    if (n_runs <= 0) return hipSuccess;
    if (n_bins < 1 || n_bins > BSIG_SCALED_MAX_BINS) return hipErrorInvalidValue;
    return launch_tiles(scaled_form(threads, coverage, !wide && P.packed_half != 0, wide, !wide && segmented, P.tile_cells,
                                    !coverage && P.ss ? 2 : 1, n_bins),
                        R, P, items, n_items, runs, n_runs, windows, resolve_first, out, st, n_bins);
}

// ---- capped 5' ends ------------------------------------------------------------------------------------------------
// one k_capped_tiles instantiation by its run-time choices (n_acc: accumulators per row, 0 without bins)
TileForm capped_form(int threads, bool half, bool wide, bool binned, int tile_cells, int rows, int n_acc)
{
    const auto f = [&](void (*k)(BSIG_TILE_PARAMS(int32_t), int, int, uint32_t, int, int), const char *name) {
        return TileForm{reinterpret_cast<const void *>(k), name, threads,
                        (size_t)hist_lds(kHistEnds, wide, tile_cells, binned ? rows * n_acc : 0).total * 4, BSIG_MODE_PROFILE};
    };
#define BSIG_CN(NT_, K_, W_, B_) f(k_capped_tiles<NT_, K_, (W_) != 0, (B_) != 0>, "k_capped_tiles<" #NT_ "," #K_ ",wide=" #W_ ",binned=" #B_ ">")
#define BSIG_CC(NT_) do { if (wide) { if (binned) return BSIG_CN(NT_, kHistEnds, 1, 1); \
                                      return BSIG_CN(NT_, kHistEnds, 1, 0); } \
                          if (half) { if (binned) return BSIG_CN(NT_, kHistEndsHalf, 0, 1); \
                                      return BSIG_CN(NT_, kHistEndsHalf, 0, 0); } \
                          if (binned) return BSIG_CN(NT_, kHistEnds, 0, 1); \
                          return BSIG_CN(NT_, kHistEnds, 0, 0); } while (0)
    if (threads == 64) BSIG_CC(64);
    if (threads == 128) BSIG_CC(128);
    if (threads == 256) BSIG_CC(256);
#undef BSIG_CC
#undef BSIG_CN
    return TileForm{};
}

hipError_t launch_capped_tiles(int threads, bool wide, bool binned, const BsigReadsDev &R, const BsigKParams &P,
                               const BsigWorkItem *items, int64_t n_items, const uint2 *runs, int64_t n_runs, void *windows,
                               bool resolve_first, int keep_dup, int ss_out, uint32_t bin_magic, int bin_shift, int n_acc,
                               int32_t *out, hipStream_t st)
{
    if (n_runs <= 0) return hipSuccess;
    if (keep_dup < 1 || !P.ss || P.binsize != 1 || (binned && n_acc < 1)) return hipErrorInvalidValue;
    return launch_tiles(capped_form(threads, !wide && P.packed_half != 0, wide, binned, P.tile_cells, ss_out ? 2 : 1, n_acc),
                        R, P, items, n_items, runs, n_runs, windows, resolve_first, out, st, keep_dup, ss_out, bin_magic, bin_shift,
                        n_acc);
}

hipError_t launch_make_ptab(const BsigReadsDev &R, const BsigKParams &P, uint8_t *out, hipStream_t st)
{
    hipLaunchKernelGGL(k_make_ptab, dim3(1), dim3(128), 0, st, R, P, out);
    return hipGetLastError();
}

hipError_t launch_make_p5h(const uint32_t *fm, const uint32_t *fmtab, int64_t n, int64_t cap, uint16_t *out, hipStream_t st)
{
    if (cap <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_make_p5h, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, st, fm, fmtab, n, cap, out);
    return hipGetLastError();
}

hipError_t launch_make_short_p5h(const int32_t *pos, const uint32_t *fm, int span_shift, int64_t n, int64_t cap, const uint32_t *idx,
                                 uint64_t n_buckets, int kshift, const uint32_t *ref_unit0, const uint32_t *ref_units, int n_ref,
                                 uint16_t *out, int *bad, hipStream_t st)
{
    if (cap <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_make_short_p5h, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, st, pos, fm, span_shift, n, cap, idx,
                       n_buckets, kshift, ref_unit0, ref_units, n_ref, out, bad);
    return hipGetLastError();
}

hipError_t launch_resolve(const BsigReadsDev &R, const BsigKParams &P, int mode, const BsigWorkItem *items,
                          int64_t n_items, void *windows, hipStream_t st)
{
    if (n_items <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_resolve, dim3((unsigned)((n_items * BSIG_MAX_CLASSES + 255) / 256)), dim3(256), 0, st,
                       R, P, mode, items, n_items, (uint2 *)windows);
    return hipGetLastError();
}

hipError_t launch_count_heavy(const void *windows, int64_t n_items, int64_t heavy_reads,
                              unsigned long long *count, hipStream_t st)
{
    if (n_items <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_count_heavy, dim3((unsigned)((n_items + 255) / 256)), dim3(256), 0, st,
                       (const uint2 *)windows, n_items, heavy_reads, count);
    return hipGetLastError();
}

hipError_t launch_cigar_end(int64_t n, const int32_t *pos, const uint16_t *flag, const int64_t *cigar_off,
                            const uint32_t *cigar, int32_t *end_out, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_cigar_end, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                       n, pos, flag, cigar_off, cigar, end_out);
    return hipGetLastError();
}

int64_t prep_chunks(int64_t n) { return (n + kPrepChunk - 1) / kPrepChunk; }

hipError_t launch_pair_sample(int64_t n, const int32_t *pos, const int32_t *end, const uint16_t *flag, const uint8_t *mapq,
                              uint32_t *hist, uint2 *pairs, uint32_t cap, uint32_t *n_pairs, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    // up to 1,024 chunks of 2,048 reads, evenly spread over the file (all of it up to 2 M reads)
    const int64_t chunks = prep_chunks(n);
    const int64_t stride = std::max<int64_t>(1, chunks / 1024);
    const int64_t blocks = (chunks + stride - 1) / stride;
    hipLaunchKernelGGL(k_pair_sample, dim3((unsigned)blocks), dim3(kPrepThreads), 0, st, n, stride, pos, end, flag, mapq, hist);
    hipLaunchKernelGGL(k_pair_compact, dim3((1u << 20) / 256), dim3(256), 0, st, hist, 1u << 20, pairs, cap, n_pairs);
    return hipGetLastError();
}

hipError_t launch_codemap_fill(const uint32_t *fmtab, int n_codes, uint16_t *codemap, hipStream_t st)
{
    if (n_codes <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_codemap_fill, dim3((unsigned)((n_codes + 255) / 256)), dim3(256), 0, st, fmtab, n_codes, codemap);
    return hipGetLastError();
}

hipError_t launch_span_hist(int64_t n, int32_t n_ref, const int64_t *ref_off, const uint32_t *ref_units, const int32_t *pos,
                            const int32_t *end, const uint16_t *flag, const uint8_t *mapq, const uint16_t *codemap,
                            uint32_t *chunk_counts, int32_t *maxspan, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_span_hist, dim3((unsigned)prep_chunks(n)), dim3(kPrepThreads), 0, st,
                       n, n_ref, ref_off, ref_units, pos, end, flag, mapq, codemap, chunk_counts, maxspan);
    return hipGetLastError();
}

hipError_t launch_chunk_scan(int64_t n_chunks, const uint32_t *counts, uint64_t *chunk_base, uint64_t *totals, hipStream_t st)
{
    hipLaunchKernelGGL(k_chunk_scan, dim3(1), dim3(kScanThreads), 0, st, n_chunks, counts, chunk_base, totals);
    return hipGetLastError();
}

hipError_t launch_scatter(int64_t n, int32_t n_ref, const int64_t *ref_off, const uint32_t *ref_unit0,
                          const uint32_t *ref_units, const int32_t *pos, const int32_t *end,
                          const uint16_t *flag, const uint8_t *mapq, const int32_t *tlen, const uint16_t *codemap,
                          const uint64_t *chunk_base, const ScatterPtrs &S, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    ScatterOut O;
    for (int c = 0; c < BSIG_MAX_CLASSES; ++c) {
        O.pos[c] = S.pos[c]; O.end[c] = S.end[c]; O.fm[c] = S.fm[c]; O.tlen[c] = S.tlen[c];
        O.gb[c] = S.gb[c]; O.kshift[c] = S.kshift[c];
    }
    hipLaunchKernelGGL(k_scatter, dim3((unsigned)prep_chunks(n)), dim3(kPrepThreads), 0, st,
                       n, n_ref, ref_off, ref_unit0, ref_units, pos, end, flag, mapq, tlen, codemap, chunk_base, O);
    return hipGetLastError();
}

hipError_t launch_build_idx(int64_t n, const uint32_t *gb, uint64_t n_buckets, uint32_t *idx, hipStream_t st)
{
    const uint64_t total = n_buckets + 1;
    hipLaunchKernelGGL(k_build_idx, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                       n, gb, n_buckets, idx);
    return hipGetLastError();
}

hipError_t launch_checksum(const void *words, uint64_t n_words, uint64_t salt, unsigned long long *acc, hipStream_t st)
{
    if (n_words == 0) return hipSuccess;
    const unsigned blocks = (unsigned)std::min<uint64_t>((n_words + 255) / 256, 256 * 32);
    hipLaunchKernelGGL(k_checksum, dim3(blocks), dim3(256), 0, st, (const uint32_t *)words, n_words, salt, acc);
    return hipGetLastError();
}

hipError_t launch_check_idx(const uint32_t *idx, uint64_t n_buckets, uint32_t n_reads, int *bad, hipStream_t st)
{
    hipLaunchKernelGGL(k_check_idx, dim3((unsigned)((n_buckets + 1 + 255) / 256)), dim3(256), 0, st, idx, n_buckets, n_reads, bad);
    return hipGetLastError();
}

hipError_t launch_visits(const BsigReadsDev &R, const BsigKParams &P, int mode, const BsigWorkItem *items,
                         int64_t n_items, unsigned long long *acc, hipStream_t st)
{
    if (n_items <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_visits, dim3((unsigned)((n_items + 255) / 256)), dim3(256), 0, st,
                       R, P, mode, items, n_items, acc);
    return hipGetLastError();
}

}  // namespace bsig

namespace { __global__ void k_warm_pileup() {} }
// loads this file's code object onto the current device (first launch of a process: ~10 ms per code object)
hipError_t bsig::warm_pileup_module(hipStream_t st)
{
    hipLaunchKernelGGL(k_warm_pileup, dim3(1), dim3(64), 0, st);
    return hipGetLastError();
}

extern "C" int bsig_debug_set_resolve_min(long long n_tiles);     // runtime.hip
extern "C" int bsig_debug_set_knob(int which, int value)
{
    if (which == 4) return bsig_debug_set_resolve_min(value);
    if (which < 0 || which >= 7 || value < 0) return -1;
    bsig::g_knobs[which] = value;
    return 0;
}

// (debug, tests: the launch log.  buf == NULL: cap 1 turns it on, cap 0 off, either way empty.  With a buffer: the names
// of the pileup, overlap, sum-tiles and reduction-tiles (k_xcorr_tiles, k_frag_tiles, k_hist_tiles, k_summary_tiles,
// k_scaled_tiles, k_vplot_tiles, k_capped_tiles) kernel forms launched since the last call, one a line, as many whole lines
// as fit cap bytes with their final 0; the log is emptied.  Returns the number of names the log held.)
extern "C" int bsig_debug_launch_log(char *buf, int cap)
{
    std::lock_guard<std::mutex> lock(bsig::g_log_mu);
    const int n = bsig::g_log_names;
    if (!buf) {
        if (cap != 0 && cap != 1) return -1;
        bsig::g_log_on.store(cap, std::memory_order_relaxed);
    } else {
        if (cap < 1) return -1;
        size_t len = std::min(bsig::g_log_text.size(), (size_t)cap - 1);
        while (len > 0 && bsig::g_log_text[len - 1] != '\n') --len;
        memcpy(buf, bsig::g_log_text.data(), len);
        buf[len] = 0;
    }
    bsig::g_log_text.clear();
    bsig::g_log_names = 0;
    return n;
}

// (debug: what the compiler made of the pileup kernels the BASELINE configurations run -- registers per lane and
// scratch bytes per lane (spills: there must be none); tests/test_gpu_parity.py.  which: 0 k_profile resolved,
// 1 its 8-wave build, 2 k_profile fused, 3 k_profile_multi (8 waves, four tiles), 4 k_coverage resolved,
// 5 k_count_multi<4, 2>, 6 k_profile resolved with strands; the half form (k_profile_half): 7 resolved, 8 its build with
// one pass in flight, 9 k_profile_multi_half (8 waves, four tiles), 10 resolved with strands)
extern "C" int bsig_debug_pileup_attrs(int which, int *vgprs, int *scratch_bytes)
{
    const void *f = nullptr;
    switch (which) {
    case 0: f = reinterpret_cast<const void *>(&k_profile<64, false, 2, 1, true>); break;
    case 1: f = reinterpret_cast<const void *>(&k_profile<64, false, 2, 8, true>); break;
    case 2: f = reinterpret_cast<const void *>(&k_profile<64, false, 2, 1, false>); break;
    case 3: f = reinterpret_cast<const void *>(&k_profile_multi<false, 2, 8, 4>); break;
    case 4: f = reinterpret_cast<const void *>(&k_coverage<64, 2, true>); break;
    case 5: f = reinterpret_cast<const void *>(&k_count_multi<4, 2>); break;
    case 6: f = reinterpret_cast<const void *>(&k_profile<64, true, 2, 1, true>); break;
    case 7: f = reinterpret_cast<const void *>(&k_profile_half<64, false, 2, 1, true>); break;
    case 8: f = reinterpret_cast<const void *>(&k_profile_half<64, false, 1, 1, true>); break;
    case 9: f = reinterpret_cast<const void *>(&k_profile_multi_half<false, 2, 8, 4>); break;
    case 10: f = reinterpret_cast<const void *>(&k_profile_half<64, true, 2, 1, true>); break;
    default: return 1;
    }
    hipFuncAttributes a;
    if (hipFuncGetAttributes(&a, f) != hipSuccess) return 2;
    if (vgprs) *vgprs = a.numRegs;
    if (scratch_bytes) *scratch_bytes = (int)a.localSizeBytes;
    return 0;
}
#ifdef BSIG_STAMPS
extern "C" int bsig_debug_set_stamp_buffer(void *buf)
{
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_stamp_buf), &buf, sizeof(buf));
}
extern "C" int bsig_debug_set_ablate(int bits)
{
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_ablate), &bits, sizeof(bits));
}
#endif
