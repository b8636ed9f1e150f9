// What the kernels over a set's base table share (nucleotides.hip: k_nuc_tiles, sites.hip: k_site_tiles): the table, the
// query and the ranges as a kernel takes them, the search of a tile's range, and the building of a tile's image in LDS -- the
// zeroing, the read window's two binary searches and the wave-a-read, lane-a-base CIGAR walk.  Device code, local to the file
// that includes this (no relocatable device code).
#ifndef BSIG_NUCWALK_H
#define BSIG_NUCWALK_H
#include <hip/hip_runtime.h>

#include "nucmath.h"

namespace {

constexpr int kNucThreads = 256;        // four waves: each takes every fourth read of the tile's window
constexpr int kNucWaves = kNucThreads / 64;

struct NucTable {
    const int32_t *pos, *endmax;
    const uint32_t *fm;
    const int64_t *cig_off, *seq_off;
    const uint32_t *cigar;
    const uint8_t *seq, *qual;
    const int64_t *ref_off;
    int32_t n_ref;
};
struct NucQuery {
    int32_t mapqual;
    uint32_t requiredF, filteredF;
    uint32_t min_qual;
};
struct NucRanges {
    int64_t n;
    const int64_t *tile_off;        // n + 1: the first tile of every range
    const int64_t *cell_off;        // n + 1: its first cell
    const int32_t *rid, *loc, *len, *strand;
};

// a read's flag / mapq filter: the rule of every other call (kernels.hip: fm_rejected), and flag 0x4
__device__ __forceinline__ bool nuc_rejected(const NucQuery &Q, uint32_t fm)
{
    const uint32_t nf = ~(fm & 0xFFFFu);
    const int mapq = (int)((fm >> 16) & 0xFFu);
    return ((fm & 0x4u) != 0u) | (mapq < Q.mapqual) | ((Q.requiredF & nf) != 0u) | ((Q.filteredF & nf) == 0u);
}

// the tile's range: the largest i with tile_off[i] <= the tile (ranges without tiles share their offset with the next
// range that has some: the largest is the one that holds the tile)
// (the three searches of a tile are made by its first thread and handed round through LDS: found, three entries)
// Every thread of the workgroup must call it.
__device__ __forceinline__ int64_t nuc_tile_range(const NucRanges &G, int64_t tile, int64_t *found)
{
    if (threadIdx.x == 0) {
        int64_t lo = 0, hi = G.n - 1;
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (G.tile_off[mid] <= tile) lo = mid; else hi = mid - 1;
        }
        found[0] = lo;
    }
    __syncthreads();
    return found[0];
}

// The tile's image: the bases [a, a + w) of reference `ref` as [plane][channel][base] int32 counters in img (one plane, two
// with SS; rows of kNucTile cells, cell j of a row is base a + j), counted from the table.  `minus`: the tile's range is a '-'
// range (which reads are sense).  Zeroes img, finds the tile's read window, walks the reads; returns behind the barrier that
// ends the walk.  found: the three entries nuc_tile_range was given.  Every thread of the workgroup must call it.
template <bool SS>
__device__ __forceinline__ void nuc_tile_image(const NucTable &T, const NucQuery &Q, int32_t ref, int64_t a, int32_t w, bool minus,
                                               int32_t *img, int64_t *found)
{
    constexpr int kPlanes = SS ? 2 : 1;
    constexpr int kImage = kPlanes * bsig::kNucChannels * bsig::kNucTile;
    constexpr int32_t kNucTile = bsig::kNucTile;
    constexpr int kNucChannels = bsig::kNucChannels;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t bnd = a + w;                                      // the tile's bases are [a, bnd) of the reference
    for (int c = tid; c < kImage; c += kNucThreads) img[c] = 0;
    const bool known = w > 0 && ref >= 0 && ref < T.n_ref;
    if (tid == 0 && known) {
        const int64_t r0 = T.ref_off[ref], r1 = T.ref_off[ref + 1];
        // the window: endmax is clamped to int32, so is what it is compared with (a superset; every read checks its extent)
        const int64_t a32 = a > 0x7FFFFFFF ? 0x7FFFFFFF : a;
        int64_t ka = r0, kb = r1;
        for (int64_t hi = r1; ka < hi;) {
            const int64_t mid = (ka + hi) >> 1;
            if ((int64_t)T.endmax[mid] < a32) ka = mid + 1; else hi = mid;
        }
        for (int64_t lo = ka; lo < kb;) {           // (lo never passes kb: the loop ends with lo == kb, the first pos >= bnd)
            const int64_t mid = (lo + kb) >> 1;
            if ((int64_t)T.pos[mid] < bnd) lo = mid + 1; else kb = mid;
        }
        found[1] = ka;
        found[2] = kb;
    }
    __syncthreads();
    if (known) {
        const int64_t ka = found[1], kb = found[2];
        for (int64_t k = ka + wave; k < kb; k += kNucWaves) {
            const uint32_t fm = T.fm[k];
            if (nuc_rejected(Q, fm)) continue;
            // sense: the read's 0x10 bit agrees with the range's strand, '*' counted as '+' (as bamCount splits)
            const int plane = SS && (((fm & 0x10u) != 0u) != minus) ? 1 : 0;
            int32_t *rows = img + plane * kNucChannels * kNucTile;
            const int64_t c0 = T.cig_off[k], c1 = T.cig_off[k + 1];
            const int64_t s0 = T.seq_off[k], l_seq = T.seq_off[k + 1] - s0;
            int64_t r = T.pos[k], q = 0;
            for (int64_t c = c0; c < c1 && r < bnd; ++c) {
                const uint32_t word = T.cigar[c];
                const uint32_t op = word & 15u;
                const int64_t L = (int64_t)(word >> 4);
                // the operation clipped to the tile
                const int64_t x0 = r > a ? r : a, x1 = r + L < bnd ? r + L : bnd;
                if (bsig::nuc_op_aligns(op)) {
                    for (int64_t x = x0 + lane; x < x1; x += 64) {
                        const int64_t qi = q + (x - r);
                        uint32_t ch = 4u;           // a base the sequence does not hold: N, its quality missing
                        bool pass = true;
                        if (qi < l_seq) {
                            const int64_t g = s0 + qi;
                            const uint32_t byte = T.seq[g >> 1];
                            const uint32_t ql = T.qual[g];
                            ch = bsig::nuc_channel((g & 1) ? byte & 15u : byte >> 4);
                            pass = ql == 0xFFu || ql >= Q.min_qual;
                        }
                        if (pass) atomicAdd(&rows[ch * kNucTile + (int32_t)(x - a)], 1);
                    }
                } else if (op == 2u) {
                    for (int64_t x = x0 + lane; x < x1; x += 64) atomicAdd(&rows[bsig::kNucDeletion * kNucTile + (int32_t)(x - a)], 1);
                }
                if (bsig::nuc_op_moves_ref(op)) r += L;
                if (bsig::nuc_op_moves_query(op)) q += L;
            }
        }
    }
    __syncthreads();
}

}  // namespace
#endif
