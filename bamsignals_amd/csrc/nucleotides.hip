// Nucleotide counts: what the reads SAY at every base of a range -- A / C / G / T / N / deletion -- counted on the GPU from the
// base table a set with bases keeps (runtime_internal.h: bsig_reads::BaseTable).  include/bamsignals_abi.h holds the
// semantics; nucmath.h the plain arithmetic.
//
// The table (bases_from_columns): the reads in BAM order with pos, endmax, flag | mapq << 16 and the offsets of their
// operations and bases, then the operations, the nibbles tightly packed and a quality byte a base, all in the set's own pool.
// endmax -- the running maximum of the reads' last bases within a reference -- is made on the host from the CIGAR columns
// (one pass over the operations).  A device decode brings the table as one piece per chunk of the inflated stream
// (devdecode.hip: chunk_bases); bases_from_device puts the pieces one behind the other -- offsets rebased, a piece that begins
// on an odd nibble shifted by four bits -- and makes endmax from the end column k_bam_extract wrote.
//
// The query (nucleotides_query): ONE launch.
//   k_nuc_tiles   a workgroup of four waves takes a TILE: at most kNucTile consecutive bases of one range (the tile's range by
//                 a binary search in the ranges' tile offsets).  The tile's image -- [plane][channel][base] int32 counters,
//                 one plane, two with ss -- lives in LDS: rows of consecutive bases, so the 64 lanes of a wave that count 64
//                 consecutive bases of a read land on 64 consecutive dwords of at most five rows, one lane a bank; with
//                 [base][channel] the lanes would stand 24 bytes apart and pile onto a third of the banks.
//                 The reads that can touch the tile are [first read whose endmax >= tile start, first read whose pos > tile
//                 end) of the tile's reference: two binary searches.  A WAVE takes a read, a LANE takes a base: the read's
//                 index is wave-uniform (readfirstlane), so its table row and its operations are scalar loads and the two
//                 cursors stay in scalar registers; an M / = / X operation is clipped to the tile and the lanes stride over
//                 what is left -- 32 consecutive bytes of nibbles, 64 consecutive quality bytes, 64 consecutive LDS cells --;
//                 a D adds to the deletion row the same way; the walk ends where the cursor passes the tile's end.
//                 A tile owns its cells: the image leaves with plain coalesced stores (zeros included: no zeroing pass over
//                 the result, no global atomics), and the drain does a '-' range's reversal and complement.  The rows of a
//                 range start wherever 4 * len puts them, so the stores are dwords, not 16-byte vectors.
// All counters are integer adds: the result does not depend on the order in which the GPU runs them.
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <vector>

#include "nucleotides.h"
#include "nucwalk.h"

using bsig::fail;
using bsig::kNucChannels;
using bsig::kNucTile;

namespace {

// (the table, the query and the ranges as the kernels take them, and the walk into a tile's image: nucwalk.h)

template <bool SS>
__global__ __launch_bounds__(kNucThreads) void k_nuc_tiles(NucTable T, NucQuery Q, NucRanges G, int32_t *__restrict__ out)
{
    constexpr int kPlanes = SS ? 2 : 1;
    constexpr int kImage = kPlanes * kNucChannels * kNucTile;
    __shared__ int32_t img[kImage];
    __shared__ int64_t found[3];
    const int tid = threadIdx.x;
    const int64_t tile = blockIdx.x;
    const int64_t i = nuc_tile_range(G, tile, found);
    const int64_t width = G.len[i];
    const int64_t rel0 = (tile - G.tile_off[i]) * kNucTile;         // the tile's first base within its range
    const int64_t left = width - rel0;
    const int32_t w = (int32_t)(left < kNucTile ? left : kNucTile);
    const bool minus = G.strand[i] < 0;
    // the image of the tile's bases (nucwalk.h): the zeroing, the read window, the walk
    nuc_tile_image<SS>(T, Q, G.rid[i], (int64_t)G.loc[i] + rel0, w, minus, img, found);
    // the drain: the tile's cells of the range's [plane][channel][position] block, a '-' range mirrored and complemented
    int32_t *__restrict__ cells = out + G.cell_off[i];
    for (int p = 0; p < kPlanes; ++p)
        for (uint32_t ch = 0; ch < (uint32_t)kNucChannels; ++ch) {
            const int32_t *row = img + (p * kNucChannels + (int)ch) * kNucTile;
            const uint32_t to = minus ? bsig::nuc_complement(ch) : ch;
            int32_t *dst = cells + ((int64_t)p * kNucChannels + to) * width;
            for (int32_t j = tid; j < w; j += kNucThreads) dst[minus ? width - 1 - (rel0 + j) : rel0 + j] = row[j];
        }
}

// ---- the table from a device decode's pieces -----------------------------------------------------------------------------------
// a piece's chunk-local offsets as the table's: each plus what the pieces before it hold
__global__ __launch_bounds__(kNucThreads) void k_nuc_offsets(int64_t n, const int64_t *__restrict__ cig_off, int64_t add_ops,
                                                             const int64_t *__restrict__ seq_off, int64_t add_bases,
                                                             int64_t *__restrict__ o_cig_off, int64_t *__restrict__ o_seq_off)
{
    const int64_t k = (int64_t)blockIdx.x * kNucThreads + threadIdx.x;
    if (k >= n) return;
    o_cig_off[k] = cig_off[k] + add_ops;
    o_seq_off[k] = seq_off[k] + add_bases;
}

// n_src bytes of nibbles (a piece that starts on its own byte) to a destination that starts in the LOW half of dst[0]: dst[0]
// keeps its high half, dst[j] for j >= 1 takes the low half of src[j - 1] and the high half of src[j]; dst[n_src] ends the
// piece with the low half of src[n_src - 1] (zero where the piece's last nibble is padding).  One thread a destination byte;
// the pieces are copied one after the other on one stream, so dst[0]'s high half stands when this runs
__global__ __launch_bounds__(kNucThreads) void k_nuc_shift_nibbles(const uint8_t *__restrict__ src, int64_t n_src, uint8_t *__restrict__ dst)
{
    const int64_t j = (int64_t)blockIdx.x * kNucThreads + threadIdx.x;
    if (j > n_src) return;
    const uint32_t hi = j == 0 ? (uint32_t)dst[0] & 0xF0u : ((uint32_t)src[j - 1] << 4) & 0xF0u;
    const uint32_t lo = j < n_src ? (uint32_t)src[j] >> 4 : 0u;
    dst[j] = (uint8_t)(hi | lo);
}

}  // namespace

namespace bsig {

int nucleotides_rule(int32_t min_base_qual)
{
    if (min_base_qual < 0 || min_base_qual > kNucMaxBaseQual)
        return fail(BSIG_ERR_ARG, "min_base_qual must lie between 0 and %d (%d given)", (int)kNucMaxBaseQual, (int)min_base_qual);
    return BSIG_OK;
}

int bases_from_columns(bsig_ctx *ctx, bsig_reads *R, const bsig_columns *cols, const bsig_base_columns *bases)
{
    hipStream_t st = ctx->stream;
    HIP_TRY(hipSetDevice(ctx->device));
    bsig_reads::BaseTable &B = R->btab;
    B = bsig_reads::BaseTable{};
    B.present = true;
    const int64_t n = cols->n_reads;
    const int32_t n_ref = cols->n_ref;
    if (n <= 0 || n_ref <= 0) return BSIG_OK;           // (an empty set: an empty table)
    const int64_t n_ops = cols->cigar_off[n], n_bases = bases->seq_off[n];
    // pos, endmax and flag | mapq << 16 of every read
    std::vector<int32_t> endmax((size_t)n);
    std::vector<uint32_t> fm((size_t)n);
    for (int32_t r = 0; r < n_ref; ++r) {
        int32_t run = INT32_MIN;
        for (int64_t k = cols->ref_off[r]; k < cols->ref_off[r + 1]; ++k) {
            const uint32_t *ops = cols->cigar + cols->cigar_off[k];
            const int64_t span = nuc_ref_span(cols->cigar_off[k + 1] - cols->cigar_off[k], [&](int64_t c) { return ops[c]; });
            run = std::max(run, nuc_clamped_end(cols->pos[k], span));
            endmax[(size_t)k] = run;
            fm[(size_t)k] = (uint32_t)cols->flag[k] | ((uint32_t)cols->mapq[k] << 16);
        }
    }
    int32_t *d_pos, *d_endmax;
    uint32_t *d_fm, *d_cigar;
    int64_t *d_cig_off, *d_seq_off, *d_ref_off;
    uint8_t *d_seq, *d_qual;
    const size_t seq_bytes = (size_t)((n_bases + 1) / 2);
    HIP_TRY(R->pool.alloc(&d_pos, (size_t)n));
    HIP_TRY(R->pool.alloc(&d_endmax, (size_t)n));
    HIP_TRY(R->pool.alloc(&d_fm, (size_t)n));
    HIP_TRY(R->pool.alloc(&d_cig_off, (size_t)n + 1));
    HIP_TRY(R->pool.alloc(&d_seq_off, (size_t)n + 1));
    HIP_TRY(R->pool.alloc(&d_cigar, (size_t)std::max<int64_t>(n_ops, 1)));
    HIP_TRY(R->pool.alloc(&d_seq, std::max<size_t>(seq_bytes, 1)));
    HIP_TRY(R->pool.alloc(&d_qual, (size_t)std::max<int64_t>(n_bases, 1)));
    HIP_TRY(R->pool.alloc(&d_ref_off, (size_t)n_ref + 1));
    HIP_TRY(hipMemcpyAsync(d_pos, cols->pos, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_endmax, endmax.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_fm, fm.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_cig_off, cols->cigar_off, ((size_t)n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_seq_off, bases->seq_off, ((size_t)n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    if (n_ops) HIP_TRY(hipMemcpyAsync(d_cigar, cols->cigar, (size_t)n_ops * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    if (n_bases) {
        HIP_TRY(hipMemcpyAsync(d_seq, bases->seq, seq_bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_qual, bases->qual, (size_t)n_bases, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipMemcpyAsync(d_ref_off, cols->ref_off, ((size_t)n_ref + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));          // (endmax and fm go away)
    B.n = n; B.n_ops = n_ops; B.n_bases = n_bases;
    B.pos = d_pos; B.endmax = d_endmax; B.fm = d_fm; B.cig_off = d_cig_off; B.seq_off = d_seq_off;
    B.cigar = d_cigar; B.seq = d_seq; B.qual = d_qual; B.ref_off = d_ref_off;
    R->info.hbm_bytes = R->pool.footprint();
    return BSIG_OK;
}

int bases_from_device(bsig_ctx *ctx, bsig_reads *R, int64_t n, int32_t n_ref, const int64_t *ref_off, const int32_t *d_pos,
                      const int32_t *d_end, const uint16_t *d_flag, const uint8_t *d_mapq, const std::vector<BasePiece> &pieces)
{
    hipStream_t st = ctx->stream;
    HIP_TRY(hipSetDevice(ctx->device));
    bsig_reads::BaseTable &B = R->btab;
    B = bsig_reads::BaseTable{};
    B.present = true;
    if (n <= 0 || n_ref <= 0) return BSIG_OK;
    int64_t n_ops = 0, n_bases = 0, n_in = 0;
    for (const BasePiece &p : pieces) { n_ops += p.n_ops; n_bases += p.n_bases; n_in += p.n; }
    if (n_in != n) return fail(BSIG_ERR_DEVICE, "the base pieces hold %lld reads, the columns %lld", (long long)n_in, (long long)n);
    // endmax and flag | mapq << 16 on the host, from the columns k_bam_extract made (its end is bam_endpos - 1: the read's own
    // base for a read without a reference-consuming operation, one more than the walk's -- the window stays a superset)
    std::vector<int32_t> endmax((size_t)n);
    std::vector<uint16_t> flag((size_t)n);
    std::vector<uint8_t> mapq((size_t)n);
    std::vector<uint32_t> fm((size_t)n);
    HIP_TRY(hipMemcpyAsync(endmax.data(), d_end, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(flag.data(), d_flag, (size_t)n * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(mapq.data(), d_mapq, (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int32_t r = 0; r < n_ref; ++r) {
        int32_t run = INT32_MIN;
        for (int64_t k = ref_off[r]; k < ref_off[r + 1]; ++k) {
            run = std::max(run, endmax[(size_t)k]);
            endmax[(size_t)k] = run;
        }
    }
    for (int64_t k = 0; k < n; ++k) fm[(size_t)k] = (uint32_t)flag[(size_t)k] | ((uint32_t)mapq[(size_t)k] << 16);
    int32_t *o_pos, *o_endmax;
    uint32_t *o_fm, *o_cigar;
    int64_t *o_cig_off, *o_seq_off, *o_ref_off;
    uint8_t *o_seq, *o_qual;
    const size_t seq_bytes = (size_t)((n_bases + 1) / 2);
    HIP_TRY(R->pool.alloc(&o_pos, (size_t)n));
    HIP_TRY(R->pool.alloc(&o_endmax, (size_t)n));
    HIP_TRY(R->pool.alloc(&o_fm, (size_t)n));
    HIP_TRY(R->pool.alloc(&o_cig_off, (size_t)n + 1));
    HIP_TRY(R->pool.alloc(&o_seq_off, (size_t)n + 1));
    HIP_TRY(R->pool.alloc(&o_cigar, (size_t)std::max<int64_t>(n_ops, 1)));
    HIP_TRY(R->pool.alloc(&o_seq, std::max<size_t>(seq_bytes, 1) + 4));
    HIP_TRY(R->pool.alloc(&o_qual, (size_t)std::max<int64_t>(n_bases, 1)));
    HIP_TRY(R->pool.alloc(&o_ref_off, (size_t)n_ref + 1));
    HIP_TRY(hipMemcpyAsync(o_pos, d_pos, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(o_endmax, endmax.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(o_fm, fm.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(o_ref_off, ref_off, ((size_t)n_ref + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    int64_t at = 0, at_ops = 0, at_bases = 0;
    for (const BasePiece &p : pieces) {
        if (p.n <= 0) continue;
        const unsigned groups = (unsigned)((p.n + kNucThreads - 1) / kNucThreads);
        hipLaunchKernelGGL(k_nuc_offsets, dim3(groups), dim3(kNucThreads), 0, st, p.n, p.cig_off, at_ops, p.seq_off, at_bases, o_cig_off + at,
                           o_seq_off + at);
        HIP_TRY(hipGetLastError());
        if (p.n_ops) HIP_TRY(hipMemcpyAsync(o_cigar + at_ops, p.cigar, (size_t)p.n_ops * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
        if (p.n_bases) {
            HIP_TRY(hipMemcpyAsync(o_qual + at_bases, p.qual, (size_t)p.n_bases, hipMemcpyDeviceToDevice, st));
            const int64_t src_bytes = (p.n_bases + 1) / 2;
            if (!(at_bases & 1)) {
                HIP_TRY(hipMemcpyAsync(o_seq + at_bases / 2, p.seq, (size_t)src_bytes, hipMemcpyDeviceToDevice, st));
            } else {
                // the piece begins in the low half of a byte the piece before it wrote: every byte of it moves up four bits
                hipLaunchKernelGGL(k_nuc_shift_nibbles, dim3((unsigned)((src_bytes + 1 + kNucThreads - 1) / kNucThreads)), dim3(kNucThreads), 0, st,
                                   p.seq, src_bytes, o_seq + at_bases / 2);
                HIP_TRY(hipGetLastError());
            }
        }
        at += p.n; at_ops += p.n_ops; at_bases += p.n_bases;
    }
    const int64_t closing[2] = {n_ops, n_bases};
    HIP_TRY(hipMemcpyAsync(o_cig_off + n, &closing[0], sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(o_seq_off + n, &closing[1], sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));          // (the host arrays go away)
    B.n = n; B.n_ops = n_ops; B.n_bases = n_bases;
    B.pos = o_pos; B.endmax = o_endmax; B.fm = o_fm; B.cig_off = o_cig_off; B.seq_off = o_seq_off;
    B.cigar = o_cigar; B.seq = o_seq; B.qual = o_qual; B.ref_off = o_ref_off;
    R->info.hbm_bytes = R->pool.footprint();
    return BSIG_OK;
}

int nucleotides_query(const bsig_reads *R, int64_t n, const int32_t *rid, const int32_t *loc, const int32_t *len, const int32_t *strand,
                      int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t min_base_qual, int32_t ss, int32_t *out_dev,
                      int32_t *out_host)
{
    if (!R) return fail(BSIG_ERR_ARG, "reads is NULL");
    if (const int rc = nucleotides_rule(min_base_qual)) return rc;
    if (!R->btab.present)
        return fail(BSIG_ERR_ARG, R->spliced ? "nucleotide counts need reads with bases: a spliced set keeps blocks, not what the reads say"
                                             : "nucleotide counts need reads with bases: a plain set keeps no base table");
    if (n < 0 || (n > 0 && (!rid || !loc || !len || !strand))) return fail(BSIG_ERR_ARG, "range arrays missing");
    std::vector<int64_t> tile_off((size_t)n + 1, 0), cell_off((size_t)n + 1, 0);
    for (int64_t i = 0; i < n; ++i) {
        if (len[i] < 0) return fail(BSIG_ERR_ARG, "range %lld has a negative width", (long long)i);
        if (rid[i] < 0 || rid[i] >= R->n_ref) return fail(BSIG_ERR_ARG, "range %lld: reference %d is not one of the set's %d", (long long)i, (int)rid[i], (int)R->n_ref);
        tile_off[(size_t)i + 1] = tile_off[(size_t)i] + nuc_tiles(len[i]);
        cell_off[(size_t)i + 1] = cell_off[(size_t)i] + nuc_cells(len[i], ss != 0);
    }
    const int64_t n_tiles = tile_off[(size_t)n], cells = cell_off[(size_t)n];
    if (n_tiles > 0x7FFFFFFF) return fail(BSIG_ERR_ARG, "a nucleotide query of more than 2^31 - 1 tiles of %d bases: ask for fewer ranges at a time", (int)kNucTile);
    if (cells == 0) return BSIG_OK;
    if (!out_dev && !out_host) return fail(BSIG_ERR_ARG, "out is NULL");
    bsig_ctx *ctx = R->ctx;
    hipStream_t st = ctx->stream;
    HIP_TRY(hipSetDevice(ctx->device));
    DevPool tmp(2.0);
    int64_t *d_tile_off, *d_cell_off;
    int32_t *d_rid, *d_loc, *d_len, *d_strand, *d_out = out_dev;
    HIP_TRY(tmp.alloc(&d_tile_off, (size_t)n + 1));
    HIP_TRY(tmp.alloc(&d_cell_off, (size_t)n + 1));
    HIP_TRY(tmp.alloc(&d_rid, (size_t)n));
    HIP_TRY(tmp.alloc(&d_loc, (size_t)n));
    HIP_TRY(tmp.alloc(&d_len, (size_t)n));
    HIP_TRY(tmp.alloc(&d_strand, (size_t)n));
    if (!d_out) HIP_TRY(tmp.alloc(&d_out, (size_t)cells));
    HIP_TRY(hipMemcpyAsync(d_tile_off, tile_off.data(), ((size_t)n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_cell_off, cell_off.data(), ((size_t)n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_rid, rid, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_loc, loc, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_len, len, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_strand, strand, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    const bsig_reads::BaseTable &B = R->btab;
    if (B.n == 0) {
        // an empty table: every cell is zero
        HIP_TRY(hipMemsetAsync(d_out, 0, (size_t)cells * sizeof(int32_t), st));
    } else {
        const NucTable T{B.pos, B.endmax, B.fm, B.cig_off, B.seq_off, B.cigar, B.seq, B.qual, B.ref_off, R->n_ref};
        const NucQuery Q{mapqual, (uint32_t)requiredF, (uint32_t)filteredF, (uint32_t)min_base_qual};
        const NucRanges G{n, d_tile_off, d_cell_off, d_rid, d_loc, d_len, d_strand};
        if (ss) hipLaunchKernelGGL(k_nuc_tiles<true>, dim3((unsigned)n_tiles), dim3(kNucThreads), 0, st, T, Q, G, d_out);
        else hipLaunchKernelGGL(k_nuc_tiles<false>, dim3((unsigned)n_tiles), dim3(kNucThreads), 0, st, T, Q, G, d_out);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(st));          // (tmp goes away)
    if (out_host) return download_to_host(ctx, d_out, out_host, (size_t)cells * sizeof(int32_t));
    return BSIG_OK;
}

}  // namespace bsig

extern "C" {

int bsig_reads_upload_bases(bsig_ctx *ctx, const bsig_columns *cols, const bsig_base_columns *bases, bsig_reads **out)
{
    if (!ctx || !cols || !bases || !out) return fail(BSIG_ERR_ARG, "NULL argument to bsig_reads_upload_bases");
    *out = nullptr;
    if (const int rc = bsig::check_columns(cols)) return rc;
    const int64_t n = cols->n_reads;
    if (n > 0) {
        if (!cols->cigar_off || !cols->cigar)
            return fail(BSIG_ERR_ARG, "reads with bases need cigar_off + cigar: an end column does not say which base lies where");
        if (!bases->seq_off) return fail(BSIG_ERR_ARG, "seq_off missing");
        if (cols->cigar_off[0] != 0 || bases->seq_off[0] != 0) return fail(BSIG_ERR_ARG, "cigar_off and seq_off must start at 0");
        for (int64_t i = 0; i < n; ++i)
            if (cols->cigar_off[i] > cols->cigar_off[i + 1] || bases->seq_off[i] > bases->seq_off[i + 1])
                return fail(BSIG_ERR_ARG, "cigar_off and seq_off must be non-decreasing");
        if (bases->seq_off[n] > 0 && (!bases->seq || !bases->qual)) return fail(BSIG_ERR_ARG, "seq or qual missing");
    }
    // the plain set first (its end column is the CIGAR's own, whatever cols->end says), then the table beside it
    bsig_columns plain = *cols;
    plain.end = nullptr;
    bsig_reads *R = nullptr;
    int rc = bsig_reads_upload(ctx, &plain, &R);
    if (rc != BSIG_OK) return rc;
    rc = bsig::bases_from_columns(ctx, R, cols, bases);
    if (rc != BSIG_OK) { bsig_reads_free(R); return rc; }
    *out = R;
    return BSIG_OK;
}

int32_t bsig_reads_has_bases(const bsig_reads *reads) { return reads && reads->btab.present ? 1 : 0; }

int64_t bsig_reads_base_table_bytes(const bsig_reads *reads)
{
    if (!reads || !reads->btab.present || reads->btab.n == 0) return 0;
    const bsig_reads::BaseTable &B = reads->btab;
    return bsig::nuc_table_bytes(B.n, B.n_ops, B.n_bases, reads->n_ref);
}

int64_t bsig_nucleotides_cells(int64_t n, const int32_t *len, int32_t ss, int64_t *off)
{
    int64_t cells = 0;
    if (off) off[0] = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (!len || len[i] < 0) return -1;
        cells += bsig::nuc_cells(len[i], ss != 0);
        if (off) off[i + 1] = cells;
    }
    return cells;
}

int bsig_reads_nucleotides(const bsig_reads *reads, int64_t n, const int32_t *rid, const int32_t *loc, const int32_t *len,
                           const int32_t *strand, int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t min_base_qual,
                           int32_t ss, int32_t *out_dev)
{
    return bsig::nucleotides_query(reads, n, rid, loc, len, strand, mapqual, requiredF, filteredF, min_base_qual, ss, out_dev, nullptr);
}

int bsig_reads_nucleotides_host(const bsig_reads *reads, int64_t n, const int32_t *rid, const int32_t *loc, const int32_t *len,
                                const int32_t *strand, int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t min_base_qual,
                                int32_t ss, int32_t *out_host)
{
    return bsig::nucleotides_query(reads, n, rid, loc, len, strand, mapqual, requiredF, filteredF, min_base_qual, ss, nullptr, out_host);
}

}  // extern "C"
