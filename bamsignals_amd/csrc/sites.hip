// Variant and mixed-allele sites: at which bases of a range do the reads disagree with a reference, or with each other?  The
// cells are those of a nucleotide count (nucleotides.hip; include/bamsignals_abi.h holds the semantics), decided where they are
// made -- in the tile's image in LDS -- so that only the sites leave the device; sitemath.h holds the decision itself.
//
// The query (sites_query): count, scan, fill.
//   k_site_tiles<SS, false>  a workgroup of four waves takes a TILE: cells [t * kNucTile, ...) of one range IN THE RANGE'S READING
//                            DIRECTION -- the tiles of a '-' range are dealt from its right end, so tile order is position order
//                            in every range.  It builds the tile's image as k_nuc_tiles does (nucwalk.h: the same function),
//                            then a wave takes 256 consecutive cells in four rounds of 64: a lane sums the planes of its cell's
//                            six rows (consecutive lanes, consecutive dwords of a row: one lane a bank), reads its reference
//                            byte (consecutive bytes) and asks bsig::site_classify.  A ballot and a popcount of the lanes below
//                            give a site its rank in the wave; the waves' totals meet in LDS.  One count per tile is written.
//   launch_gap_scan          (splice.hip) the exclusive scan of the tile counts in 64 bits, and the total
//   k_site_seg_off           seg_off[i] = the scan's value at the range's first tile
//   k_site_tiles<SS, true>   the same walk and the same decisions; a tile without sites returns before it touches LDS; a site
//                            goes to slot tile base + waves before + rank: pos, b | a << 8 and its 6 (12 with ss) counts.
// No global atomics, no order from scheduling: the same arrays every run.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>
#include <memory>
#include <vector>

#include "nucleotides.h"
#include "nucwalk.h"
#include "sites.h"
#include "splice.h"

using bsig::fail;
using bsig::kNucChannels;
using bsig::kNucTile;
using bsig::SiteParams;

namespace {

constexpr int kSiteRounds = kNucTile / kNucThreads;         // a wave's 64-cell rounds: its cells are 64 * kSiteRounds consecutive ones

inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// G.cell_off is the ranges' first BASE here (the running sum of len): where a range's reference bytes begin
template <bool SS, bool FILL>
__global__ __launch_bounds__(kNucThreads) void k_site_tiles(NucTable T, NucQuery Q, NucRanges G, SiteParams P, const uint8_t *__restrict__ ref,
                                                            uint32_t *__restrict__ tile_count, const int64_t *__restrict__ tile_base,
                                                            int64_t n_sites, int32_t *__restrict__ o_pos, int32_t *__restrict__ o_alleles,
                                                            int32_t *__restrict__ o_counts)
{
    constexpr int kPlanes = SS ? 2 : 1;
    constexpr int kImage = kPlanes * kNucChannels * kNucTile;
    const int64_t tile = blockIdx.x;
    if (FILL && tile_count[tile] == 0u) return;         // (the whole workgroup: nothing of LDS is touched)
    __shared__ int32_t img[kImage];
    __shared__ int64_t found[3];
    __shared__ uint32_t wave_total[kNucWaves];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t i = nuc_tile_range(G, tile, found);
    const int64_t width = G.len[i];
    const int64_t cell0 = (tile - G.tile_off[i]) * kNucTile;        // the tile's first cell within its range, as the range reads
    const int64_t left = width - cell0;
    const int32_t w = (int32_t)(left < kNucTile ? left : kNucTile);
    const bool minus = G.strand[i] < 0;
    // the tile's bases on the reference: a '-' range's cell p is base loc + width - 1 - p
    const int64_t a = minus ? (int64_t)G.loc[i] + width - cell0 - w : (int64_t)G.loc[i] + cell0;
    nuc_tile_image<SS>(T, Q, G.rid[i], a, w, minus, img, found);
    // ---- the decisions: cell q of the tile is column j of the image; a '-' range's channel k is row complement(k) ---------------
    const uint8_t *ref_at = ref ? ref + G.cell_off[i] + cell0 : nullptr;
    int32_t cls[kSiteRounds];
    uint32_t rank[kSiteRounds];
    uint32_t mine = 0;                      // the wave's sites so far (wave-uniform)
#pragma unroll
    for (int r = 0; r < kSiteRounds; ++r) {
        const int32_t q = (wave * kSiteRounds + r) * 64 + lane;
        int32_t k = -1;
        if (q < w) {
            const int32_t j = minus ? w - 1 - q : q;
            int64_t c[kNucChannels];
#pragma unroll
            for (uint32_t ch = 0; ch < (uint32_t)kNucChannels; ++ch) {
                const uint32_t row = minus ? bsig::nuc_complement(ch) : ch;
                int64_t v = img[row * kNucTile + j];
                if (SS) v += img[(kNucChannels + row) * kNucTile + j];
                c[ch] = v;
            }
            k = bsig::site_classify(c, ref_at ? (int32_t)ref_at[q] : -1, P);
        }
        const unsigned long long m = __ballot(k >= 0);
        cls[r] = k;
        rank[r] = mine + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        mine += (uint32_t)__popcll(m);
    }
    if (lane == 0) wave_total[wave] = mine;
    __syncthreads();
    if (!FILL) {
        if (tid == 0) {
            uint32_t sum = 0;
            for (int v = 0; v < kNucWaves; ++v) sum += wave_total[v];
            tile_count[tile] = sum;
        }
        return;
    }
    int64_t slot0 = tile_base[tile];
    for (int v = 0; v < wave; ++v) slot0 += wave_total[v];
#pragma unroll
    for (int r = 0; r < kSiteRounds; ++r) {
        if (cls[r] < 0) continue;
        const int64_t s = slot0 + rank[r];
        if (s >= n_sites) continue;         // (cannot be: the count pass made the same decisions)
        const int32_t q = (wave * kSiteRounds + r) * 64 + lane;
        const int32_t j = minus ? w - 1 - q : q;
        o_pos[s] = (int32_t)(cell0 + q);
        o_alleles[s] = cls[r];
        int32_t *cnt = o_counts + s * (kPlanes * kNucChannels);
#pragma unroll
        for (int p = 0; p < kPlanes; ++p)
#pragma unroll
            for (uint32_t ch = 0; ch < (uint32_t)kNucChannels; ++ch) {
                const uint32_t row = minus ? bsig::nuc_complement(ch) : ch;
                cnt[p * kNucChannels + (int)ch] = img[(p * kNucChannels + (int)row) * kNucTile + j];
            }
    }
}

// seg_off[i], i = 0 .. n: the scan's value at the range's first tile; ranges behind the last tile, and entry n, take the total
__global__ __launch_bounds__(kNucThreads) void k_site_seg_off(int64_t n, const int64_t *__restrict__ tile_off, int64_t n_tiles,
                                                              const int64_t *__restrict__ tile_base, const int64_t *__restrict__ total,
                                                              int64_t *__restrict__ seg_off)
{
    const int64_t k = (int64_t)blockIdx.x * kNucThreads + threadIdx.x;
    if (k > n) return;
    const int64_t t = tile_off[k];
    seg_off[k] = t < n_tiles ? tile_base[t] : *total;
}

template <bool FILL>
void launch_site_tiles(bool ss, unsigned n_tiles, hipStream_t st, const NucTable &T, const NucQuery &Q, const NucRanges &G, const SiteParams &P,
                       const uint8_t *ref, uint32_t *tile_count, const int64_t *tile_base, int64_t n_sites, int32_t *o_pos,
                       int32_t *o_alleles, int32_t *o_counts)
{
    if (ss)
        hipLaunchKernelGGL((k_site_tiles<true, FILL>), dim3(n_tiles), dim3(kNucThreads), 0, st, T, Q, G, P, ref, tile_count, tile_base, n_sites, o_pos,
                           o_alleles, o_counts);
    else
        hipLaunchKernelGGL((k_site_tiles<false, FILL>), dim3(n_tiles), dim3(kNucThreads), 0, st, T, Q, G, P, ref, tile_count, tile_base, n_sites, o_pos,
                           o_alleles, o_counts);
}

}  // namespace

namespace bsig {

int sites_rule(int32_t min_base_qual, int32_t min_depth, int32_t min_alt, int32_t frac_num, int32_t frac_den, int32_t alt_mask)
{
    if (const int rc = nucleotides_rule(min_base_qual)) return rc;
    if (const char *why = site_rule_sentence(min_depth, min_alt, frac_num, frac_den, alt_mask))
        return fail(BSIG_ERR_ARG, "%s (min_depth %d, min_alt %d, frac %d / %d, alt_mask 0x%X given)", why, (int)min_depth, (int)min_alt,
                    (int)frac_num, (int)frac_den, (unsigned)alt_mask);
    return BSIG_OK;
}

int sites_ref_rule(int64_t n, const int32_t *len, const uint8_t *ref)
{
    if (!ref || !len) return BSIG_OK;
    int64_t at = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (len[i] <= 0) continue;
        uint32_t bad = 0;
        for (int64_t p = 0; p < len[i]; ++p) bad |= (uint32_t)(ref[at + p] > (uint8_t)kSiteRefN);
        if (bad)
            for (int64_t p = 0; p < len[i]; ++p)
                if (ref[at + p] > (uint8_t)kSiteRefN)
                    return fail(BSIG_ERR_ARG, "ref: code %d at cell %lld of range %lld is none of the channel codes 0 .. 4", (int)ref[at + p],
                                (long long)p, (long long)i);
        at += len[i];
    }
    return BSIG_OK;
}

int sites_query(const bsig_reads *R, int64_t n, const int32_t *rid, const int32_t *loc, const int32_t *len, const int32_t *strand,
                int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t min_base_qual, int32_t ss, const uint8_t *ref,
                const SiteParams &prm, bsig_sites_result *out)
{
    if (!R || !out) return fail(BSIG_ERR_ARG, "NULL argument");
    if (const int rc = sites_rule(min_base_qual, prm.min_depth, prm.min_alt, prm.frac_num, prm.frac_den, (int32_t)prm.alt_mask)) return rc;
    if (!R->btab.present)
        return fail(BSIG_ERR_ARG, R->spliced ? "nucleotide counts need reads with bases: a spliced set keeps blocks, not what the reads say"
                                             : "nucleotide counts need reads with bases: a plain set keeps no base table");
    if (n < 0 || (n > 0 && (!rid || !loc || !len || !strand))) return fail(BSIG_ERR_ARG, "range arrays missing");
    std::vector<int64_t> tile_off((size_t)n + 1, 0), base_off((size_t)n + 1, 0);
    for (int64_t i = 0; i < n; ++i) {
        if (len[i] < 0) return fail(BSIG_ERR_ARG, "range %lld has a negative width", (long long)i);
        if (rid[i] < 0 || rid[i] >= R->n_ref) return fail(BSIG_ERR_ARG, "range %lld: reference %d is not one of the set's %d", (long long)i, (int)rid[i], (int)R->n_ref);
        tile_off[(size_t)i + 1] = tile_off[(size_t)i] + nuc_tiles(len[i]);
        base_off[(size_t)i + 1] = base_off[(size_t)i] + len[i];
    }
    const int64_t n_tiles = tile_off[(size_t)n], n_bases = base_off[(size_t)n];
    if (n_tiles > 0x7FFFFFFF) return fail(BSIG_ERR_ARG, "a nucleotide query of more than 2^31 - 1 tiles of %d bases: ask for fewer ranges at a time", (int)kNucTile);
    if (const int rc = sites_ref_rule(n, len, ref)) return rc;
    out->ss = ss != 0;
    out->n_seg = n;
    out->seg_off.assign((size_t)n + 1, 0);
    for (int c = 0; c < EncodedColumns::kMaxCols; ++c) out->col[c].clear();
    const bsig_reads::BaseTable &B = R->btab;
    if (n_bases == 0 || B.n == 0) return BSIG_OK;           // (an empty table: every cell is zero, and min_depth is at least 1)
    bsig_ctx *ctx = R->ctx;
    hipStream_t st = ctx->stream;
    HIP_TRY(hipSetDevice(ctx->device));
    DevPool tmp(2.0);
    int64_t *d_tile_off, *d_base_off, *d_tile_base, *d_total, *d_seg_off;
    int32_t *d_rid, *d_loc, *d_len, *d_strand;
    uint32_t *d_tile_count;
    uint8_t *d_ref = nullptr;
    HIP_TRY(tmp.alloc(&d_tile_off, (size_t)n + 1));
    HIP_TRY(tmp.alloc(&d_base_off, (size_t)n + 1));
    HIP_TRY(tmp.alloc(&d_seg_off, (size_t)n + 1));
    HIP_TRY(tmp.alloc(&d_rid, (size_t)n));
    HIP_TRY(tmp.alloc(&d_loc, (size_t)n));
    HIP_TRY(tmp.alloc(&d_len, (size_t)n));
    HIP_TRY(tmp.alloc(&d_strand, (size_t)n));
    HIP_TRY(tmp.alloc(&d_tile_count, (size_t)n_tiles));
    HIP_TRY(tmp.alloc(&d_tile_base, (size_t)n_tiles));
    HIP_TRY(tmp.alloc(&d_total, 1));
    if (ref) HIP_TRY(tmp.alloc(&d_ref, (size_t)n_bases));
    HIP_TRY(hipMemcpyAsync(d_tile_off, tile_off.data(), ((size_t)n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_base_off, base_off.data(), ((size_t)n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_rid, rid, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_loc, loc, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_len, len, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_strand, strand, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (ref) HIP_TRY(hipMemcpyAsync(d_ref, ref, (size_t)n_bases, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));          // (the uploads are not the query's device time)
    const NucTable T{B.pos, B.endmax, B.fm, B.cig_off, B.seq_off, B.cigar, B.seq, B.qual, B.ref_off, R->n_ref};
    const NucQuery Q{mapqual, (uint32_t)requiredF, (uint32_t)filteredF, (uint32_t)min_base_qual};
    const NucRanges G{n, d_tile_off, d_base_off, d_rid, d_loc, d_len, d_strand};
    // ---- count, scan, the ranges' offsets ------------------------------------------------------------------------------
    const double t0 = now_s();
    launch_site_tiles<false>(ss != 0, (unsigned)n_tiles, st, T, Q, G, prm, d_ref, d_tile_count, nullptr, 0, nullptr, nullptr, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(launch_gap_scan(n_tiles, d_tile_count, d_tile_base, d_total, st));
    hipLaunchKernelGGL(k_site_seg_off, dim3((unsigned)((n + 1 + kNucThreads - 1) / kNucThreads)), dim3(kNucThreads), 0, st, n, d_tile_off, n_tiles,
                       d_tile_base, d_total, d_seg_off);
    HIP_TRY(hipGetLastError());
    int64_t n_sites = 0;
    HIP_TRY(hipMemcpyAsync(&n_sites, d_total, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const double t1 = now_s();
    out->seconds[0] = t1 - t0;
    if (n_sites < 0 || n_sites > n_bases) return fail(BSIG_ERR_DEVICE, "site count %lld out of range", (long long)n_sites);
    if (n_sites == 0) return BSIG_OK;
    // ---- fill: the arrays at their exact size ----------------------------------------------------------------------------
    const size_t per = (ss ? 2 : 1) * (size_t)kNucChannels;
    int32_t *d_pos, *d_alleles, *d_counts;
    HIP_TRY(tmp.alloc(&d_pos, (size_t)n_sites));
    HIP_TRY(tmp.alloc(&d_alleles, (size_t)n_sites));
    HIP_TRY(tmp.alloc(&d_counts, per * (size_t)n_sites));
    launch_site_tiles<true>(ss != 0, (unsigned)n_tiles, st, T, Q, G, prm, d_ref, d_tile_count, d_tile_base, n_sites, d_pos, d_alleles, d_counts);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    const double t2 = now_s();
    out->seconds[1] = t2 - t1;
    // ---- only the sites leave the device -----------------------------------------------------------------------------------
    const size_t elem[3] = {sizeof(int32_t), sizeof(int32_t), per * sizeof(int32_t)};
    const void *src[3] = {d_pos, d_alleles, d_counts};
    int rc = download_to_host(ctx, d_seg_off, out->seg_off.data(), ((size_t)n + 1) * sizeof(int64_t));
    for (int c = 0; c < 3 && rc == BSIG_OK; ++c) {
        out->col[c].resize((size_t)n_sites * elem[c]);
        rc = download_to_host(ctx, src[c], out->col[c].data(), out->col[c].size());
    }
    out->seconds[2] = now_s() - t2;
    if (rc == BSIG_OK && out->seg_off.back() != n_sites) rc = fail(BSIG_ERR_DEVICE, "site offsets do not add up");
    return rc;
}

}  // namespace bsig

extern "C" {

int bsig_reads_sites(const bsig_reads *reads, int64_t n, const int32_t *rid, const int32_t *loc, const int32_t *len, const int32_t *strand,
                     int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t min_base_qual, int32_t ss, const uint8_t *ref,
                     int32_t min_depth, int32_t min_alt, int32_t frac_num, int32_t frac_den, int32_t alt_mask, bsig_sites_result **result)
{
    if (!result) return fail(BSIG_ERR_ARG, "result is NULL");
    *result = nullptr;
    if (!reads) return fail(BSIG_ERR_ARG, "reads is NULL");
    std::unique_ptr<bsig_sites_result> res(new bsig_sites_result);
    const SiteParams prm{min_depth, min_alt, frac_num, frac_den, (uint32_t)alt_mask};
    const int rc = bsig::sites_query(reads, n, rid, loc, len, strand, mapqual, requiredF, filteredF, min_base_qual, ss, ref, prm, res.get());
    if (rc == BSIG_OK) *result = res.release();
    return rc;
}

int64_t bsig_sites_result_n_ranges(const bsig_sites_result *r) { return r ? r->n_seg : 0; }

int64_t bsig_sites_result_n_sites(const bsig_sites_result *r) { return r ? r->entries() : 0; }

int bsig_sites_result_copy(const bsig_sites_result *r, int64_t *seg_off, int32_t *pos, int32_t *alleles, int32_t *counts)
{
    if (!r || !seg_off) return fail(BSIG_ERR_ARG, "NULL argument");
    const size_t n = (size_t)r->entries();
    if (n && (!pos || !alleles || !counts)) return fail(BSIG_ERR_ARG, "output buffer is NULL");
    memcpy(seg_off, r->seg_off.data(), r->seg_off.size() * sizeof(int64_t));
    void *const dst[3] = {pos, alleles, counts};
    for (int c = 0; n && c < 3; ++c) memcpy(dst[c], r->col[c].data(), r->col[c].size());
    return BSIG_OK;
}

void bsig_sites_result_timing(const bsig_sites_result *r, double *t3)
{
    if (!t3) return;
    for (int k = 0; k < 3; ++k) t3[k] = r ? r->seconds[k] : 0.0;
}

void bsig_sites_result_free(bsig_sites_result *r) { delete r; }

}  // extern "C"
