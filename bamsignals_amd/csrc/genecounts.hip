// Reads per gene: every read of a spliced set classified against a gene model, counted on the GPU.
//
// The set's READ TABLE (splice.hip keeps it: the reads in BAM order, each with its blocks and flag | mapq << 16) is walked one
// read per work item against the model's flattened SEGMENT TABLES (genemodel.h: disjoint segments per reference whose value
// is a gene or kGeneAmbig; one table for all features, one per strand):
//   k_gene_classify   the read's reference (binary search in the per-reference read offsets), its table (unstranded: the one
//                     of all features; forward: its own strand's -- a second mate's strand flipped --; reverse: the other's),
//                     the reference's slice of that table.  For the first block a binary search finds the first segment that
//                     ends at or behind the block's first base; segments are walked while they begin at or before its last
//                     base; the cursor goes on to the next block (blocks ascend), GALLOPING where that block begins beyond
//                     the cursor's segment: 1, 2, 4 .. segments ahead, then a binary search in the last stride -- an intron
//                     costs the logarithm of the segments it holds.  The walk ends at once when it is ambiguous.  The read
//                     ends with one OUTCOME: the cell of its gene, or of ambiguous / no_feature / filtered / unmapped.
//                     Counting: neighbouring reads mostly share an outcome, so a wave adds once per DISTINCT outcome among
//                     its lanes: the first lane not yet counted names its outcome, a ballot finds every lane that shares
//                     it -- the run it heads and every later run of the same outcome --, that lane adds their number, and
//                     the loop goes on with the lanes left.  A gene's number goes to its cell with one 64-bit integer
//                     atomic; the four other outcomes and the wave's reads with a gene (assigned) are summed per workgroup
//                     in LDS first and reach their cells with at most five atomics per workgroup: every wave of the launch
//                     adds to those few addresses.  (Run heads alone, measured first: a mapq filter cuts the runs of a gene
//                     into pieces of two reads, each piece's neighbour an atom on the ONE filtered cell -- 65 ms for
//                     20,000,000 reads where the unfiltered query took 3.8.)  Integer adds commute: the same result on
//                     every run.
// One launch, nothing waits for anything; only the n_genes + 5 int64 cells are downloaded.
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <vector>

#include "genecounts.h"

using bsig::fail;
using bsig::GeneModel;
using bsig::GeneSegments;
using bsig::kGeneSummary;
using bsig::kGeneTables;

namespace {

constexpr int kGeneThreads = 256;       // reads per workgroup
constexpr int kWaveLanes = 64;
// the summary's cells behind the genes'
enum { kAssigned = 0, kAmbiguous = 1, kNoFeature = 2, kFiltered = 3, kUnmapped = 4 };

struct GeneQuery {
    int32_t mapqual;
    uint32_t requiredF, filteredF;
    int32_t strandedness;       // 0 unstranded, 1 forward, 2 reverse
    int32_t n_ref, n_genes;
};

// a read's flag / mapq filter: the rule of every other call (kernels.hip: fm_rejected)
__device__ __forceinline__ bool gene_rejected(const GeneQuery &Q, uint32_t fm)
{
    const uint32_t nf = ~(fm & 0xFFFFu);
    const int mapq = (int)((fm >> 16) & 0xFFu);
    return (mapq < Q.mapqual) | ((Q.requiredF & nf) != 0u) | ((Q.filteredF & nf) == 0u);
}

// the reference of read i: the largest r < n_ref with ref_off[r] <= i (references without reads share their offset with the
// next one: the largest is the one that holds the read)
__device__ __forceinline__ int32_t gene_ref_of(const int64_t *__restrict__ ref_off, int32_t n_ref, int64_t i)
{
    int32_t lo = 0, hi = n_ref - 1;
    while (lo < hi) {
        const int32_t mid = (lo + hi + 1) >> 1;
        if (ref_off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// the first segment k in [from, s1) with seg_end[k] >= base (s1 if there is none): `from` itself where it qualifies, else a
// gallop -- strides of 1, 2, 4 .. until a segment qualifies or the slice ends -- and a binary search in the last stride
__device__ __forceinline__ int64_t first_segment(const int32_t *__restrict__ seg_end, int64_t from, int64_t s1, int32_t base)
{
    if (from >= s1 || seg_end[from] >= base) return from;
    int64_t lo = from, step = 1, hi = from + 1;            // seg_end[lo] < base throughout
    while (hi < s1 && seg_end[hi] < base) {
        lo = hi;
        step <<= 1;
        hi = lo + step;
    }
    if (hi > s1) hi = s1;
    ++lo;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (seg_end[mid] < base) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// slice[(table * n_ref + r) * 2 ..]: the segments [first, last) of the set's reference r in that table, as rows of the
// device columns (the three tables back to back)
__global__ __launch_bounds__(kGeneThreads) void k_gene_classify(int64_t n, const int64_t *__restrict__ ref_off,
                                                               const uint32_t *__restrict__ blk_off, const uint32_t *__restrict__ read_fm,
                                                               const int32_t *__restrict__ bstart, const int32_t *__restrict__ bend,
                                                               int64_t n_blocks, const int64_t *__restrict__ slice,
                                                               const int32_t *__restrict__ seg_start, const int32_t *__restrict__ seg_end,
                                                               const int32_t *__restrict__ seg_value, int64_t n_seg, GeneQuery Q,
                                                               unsigned long long *__restrict__ cells)
{
    __shared__ unsigned int group_sum[kGeneSummary];
    const int64_t i = (int64_t)blockIdx.x * kGeneThreads + threadIdx.x;
    const int32_t summary0 = Q.n_genes;
    if (threadIdx.x < kGeneSummary) group_sum[threadIdx.x] = 0u;
    __syncthreads();
    int32_t code = -1;                          // the cell this read adds to; -1: no read
    if (i < n) {
        const uint32_t fm = read_fm[i];
        if (fm & 0x4u) {
            code = summary0 + kUnmapped;
        } else if (gene_rejected(Q, fm)) {
            code = summary0 + kFiltered;
        } else {
            int s = (fm & 0x10u) ? -1 : 1;
            if ((fm & 0x81u) == 0x81u) s = -s;  // a second mate lies on the other strand of its fragment
            const int table = Q.strandedness == 0 ? 0 : ((Q.strandedness == 1) == (s > 0)) ? 1 : 2;
            const int32_t r = gene_ref_of(ref_off, Q.n_ref, i);
            int64_t s0 = slice[((int64_t)table * Q.n_ref + r) * 2], s1 = slice[((int64_t)table * Q.n_ref + r) * 2 + 1];
            s1 = s1 < n_seg ? s1 : n_seg;
            int64_t b = blk_off[i], b1 = blk_off[i + 1];
            b1 = b1 < n_blocks ? b1 : n_blocks;
            constexpr int32_t kNone = -2;
            int32_t found = kNone;
            bool ambiguous = false;
            int64_t cursor = s0;
            for (; b < b1 && !ambiguous && cursor < s1; ++b) {
                const int32_t first = bstart[b], last = bend[b];
                int64_t k = first_segment(seg_end, cursor, s1, first);
                cursor = k;
                for (; k < s1 && seg_start[k] <= last; ++k) {
                    const int32_t v = seg_value[k];
                    if (v < 0 || (found != kNone && found != v)) { ambiguous = true; break; }
                    found = v;
                    cursor = k;                 // (the segment may reach into the next block)
                }
            }
            code = ambiguous ? summary0 + kAmbiguous : found == kNone ? summary0 + kNoFeature : found;
            if (code >= summary0 + kGeneSummary) code = summary0 + kAmbiguous;      // (never out of bounds)
        }
    }
    // one add per distinct outcome of the wave: `todo` is the same in every lane, so the loop is the wave's
    const int lane = threadIdx.x & (kWaveLanes - 1);
    unsigned long long todo = __ballot(code >= 0);
    const unsigned long long genes = __ballot(code >= 0 && code < summary0);
    while (todo) {
        const int first = __ffsll((long long)todo) - 1;
        const int32_t c = __shfl(code, first);
        const unsigned long long same = __ballot(code == c);
        if (lane == first) {
            const unsigned int k = (unsigned int)__popcll(same);
            if (c < summary0) atomicAdd(&cells[c], (unsigned long long)k);
            else atomicAdd(&group_sum[c - summary0], k);
        }
        todo &= ~same;
    }
    if (lane == 0 && genes) atomicAdd(&group_sum[kAssigned], (unsigned int)__popcll(genes));
    __syncthreads();
    if (threadIdx.x < kGeneSummary && group_sum[threadIdx.x]) atomicAdd(&cells[summary0 + threadIdx.x], (unsigned long long)group_sum[threadIdx.x]);
}

// the model's three tables on the query's device: made at the first query there, kept with the model
int model_on_device(const bsig_gene_model *M, bsig_ctx *ctx, const bsig_gene_model::OnDevice **out)
{
    std::lock_guard<std::mutex> lock(M->mu);
    auto it = M->dev.find(ctx->device);
    if (it != M->dev.end()) { *out = it->second.get(); return BSIG_OK; }
    std::unique_ptr<bsig_gene_model::OnDevice> D(new bsig_gene_model::OnDevice);
    const int64_t total = M->base(kGeneTables);
    const size_t cap = (size_t)std::max<int64_t>(total, 1);
    int32_t *d_start, *d_end, *d_value;
    HIP_TRY(D->pool.alloc(&d_start, cap));
    HIP_TRY(D->pool.alloc(&d_end, cap));
    HIP_TRY(D->pool.alloc(&d_value, cap));
    hipStream_t st = ctx->stream;
    for (int t = 0; t < kGeneTables; ++t) {
        const GeneSegments &S = M->host.table[t];
        const size_t bytes = (size_t)S.size() * sizeof(int32_t);
        if (!bytes) continue;
        const int64_t at = M->base(t);
        HIP_TRY(hipMemcpyAsync(d_start + at, S.start.data(), bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_end + at, S.end.data(), bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_value + at, S.value.data(), bytes, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipStreamSynchronize(st));          // (the host vectors may go away with the model)
    D->start = d_start; D->end = d_end; D->value = d_value;
    *out = D.get();
    M->dev[ctx->device] = std::move(D);
    return BSIG_OK;
}

}  // namespace

namespace bsig {

int gene_counts_rule(const bsig_gene_model *model, int32_t strandedness, const int64_t *counts, const int64_t *summary)
{
    if (!model) return fail(BSIG_ERR_ARG, "model is NULL");
    if (strandedness < 0 || strandedness > 2)
        return fail(BSIG_ERR_ARG, "strandedness must be 0 (unstranded), 1 (forward) or 2 (reverse): %d given", (int)strandedness);
    if (!summary || (model->host.n_genes > 0 && !counts)) return fail(BSIG_ERR_ARG, "counts or summary is NULL");
    return BSIG_OK;
}

int gene_counts_query(const bsig_reads *R, const bsig_gene_model *M, const int32_t *ref_map, int32_t mapqual, int32_t requiredF,
                      int32_t filteredF, int32_t strandedness, int64_t *counts, int64_t *summary)
{
    if (!R) return fail(BSIG_ERR_ARG, "reads is NULL");
    if (const int rc = gene_counts_rule(M, strandedness, counts, summary)) return rc;
    if (!R->spliced) return fail(BSIG_ERR_ARG, "gene counts need spliced reads: a plain set keeps no read table");
    const GeneModel &G = M->host;
    if (!ref_map && G.n_ref != R->n_ref)
        return fail(BSIG_ERR_ARG, "the gene model has %d references, the reads have %d", (int)G.n_ref, (int)R->n_ref);
    const int32_t n_ref = R->n_ref;
    if (ref_map)
        for (int32_t r = 0; r < n_ref; ++r)
            if (ref_map[r] < -1 || ref_map[r] >= G.n_ref) return fail(BSIG_ERR_ARG, "reference %d maps to none of the model's", (int)r);
    std::fill(counts, counts + (G.n_genes > 0 ? G.n_genes : 0), (int64_t)0);
    std::fill(summary, summary + kGeneSummary, (int64_t)0);
    const bsig_reads::ReadTable &T = R->rtab;
    if (T.n <= 0 || n_ref <= 0) return BSIG_OK;
    if (G.n_genes >= INT32_MAX - kGeneSummary) return fail(BSIG_ERR_ARG, "too many genes");
    bsig_ctx *ctx = R->ctx;
    hipStream_t st = ctx->stream;
    HIP_TRY(hipSetDevice(ctx->device));
    const bsig_gene_model::OnDevice *D = nullptr;
    if (const int rc = model_on_device(M, ctx, &D)) return rc;
    // the set's references' slices of the three tables
    std::vector<int64_t> slice((size_t)kGeneTables * (size_t)n_ref * 2, 0);
    for (int t = 0; t < kGeneTables; ++t)
        for (int32_t r = 0; r < n_ref; ++r) {
            const int32_t mr = ref_map ? ref_map[r] : r;
            if (mr < 0) continue;
            const GeneSegments &S = G.table[t];
            slice[((size_t)t * (size_t)n_ref + (size_t)r) * 2] = M->base(t) + S.ref_off[(size_t)mr];
            slice[((size_t)t * (size_t)n_ref + (size_t)r) * 2 + 1] = M->base(t) + S.ref_off[(size_t)mr + 1];
        }
    DevPool tmp(2.0);
    const size_t n_cells = (size_t)G.n_genes + kGeneSummary;
    int64_t *d_slice;
    unsigned long long *d_cells;
    HIP_TRY(tmp.alloc(&d_slice, slice.size()));
    HIP_TRY(tmp.alloc(&d_cells, n_cells));
    HIP_TRY(hipMemcpyAsync(d_slice, slice.data(), slice.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_cells, 0, n_cells * sizeof(unsigned long long), st));
    const GeneQuery Q{mapqual, (uint32_t)requiredF, (uint32_t)filteredF, strandedness, n_ref, G.n_genes};
    const unsigned groups = (unsigned)((T.n + kGeneThreads - 1) / kGeneThreads);
    hipLaunchKernelGGL(k_gene_classify, dim3(groups), dim3(kGeneThreads), 0, st, T.n, T.ref_off, T.blk_off, T.fm, T.bstart, T.bend, T.n_blocks,
                       d_slice, D->start, D->end, D->value, M->base(kGeneTables), Q, d_cells);
    HIP_TRY(hipGetLastError());
    std::vector<int64_t> cells(n_cells);
    HIP_TRY(hipMemcpyAsync(cells.data(), d_cells, n_cells * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::copy(cells.begin(), cells.begin() + G.n_genes, counts);
    std::copy(cells.begin() + G.n_genes, cells.end(), summary);
    return BSIG_OK;
}

}  // namespace bsig

extern "C" {

int bsig_gene_model_create(int64_t n, const int32_t *rid, const int32_t *loc, const int32_t *len, const int32_t *strand,
                           const int32_t *gene, int32_t n_genes, int32_t n_ref, bsig_gene_model **model)
{
    if (!model) return fail(BSIG_ERR_ARG, "model is NULL");
    *model = nullptr;
    const std::string no = bsig::gene_model_refusal(n, rid, loc, len, strand, gene, n_genes, n_ref);
    if (!no.empty()) return fail(BSIG_ERR_ARG, "%s", no.c_str());
    std::unique_ptr<bsig_gene_model> M(new bsig_gene_model);
    bsig::build_gene_model(n, rid, loc, len, strand, gene, n_genes, n_ref, &M->host);
    if (M->base(kGeneTables) >= ((int64_t)1 << 31)) return fail(BSIG_ERR_ARG, "more than 2^31 segments in a gene model");
    *model = M.release();
    return BSIG_OK;
}

void bsig_gene_model_free(bsig_gene_model *model) { delete model; }

int32_t bsig_gene_model_n_genes(const bsig_gene_model *model) { return model ? model->host.n_genes : 0; }

int32_t bsig_gene_model_n_ref(const bsig_gene_model *model) { return model ? model->host.n_ref : 0; }

int64_t bsig_gene_model_n_segments(const bsig_gene_model *model, int32_t table)
{
    return model && table >= 0 && table < kGeneTables ? model->host.table[table].size() : -1;
}

int bsig_gene_model_copy_segments(const bsig_gene_model *model, int32_t table, int64_t *ref_off, int32_t *start, int32_t *end,
                                  int32_t *value)
{
    if (!model || !ref_off) return fail(BSIG_ERR_ARG, "NULL argument");
    if (table < 0 || table >= kGeneTables) return fail(BSIG_ERR_ARG, "table must be 0 (unstranded), 1 (plus) or 2 (minus): %d given", (int)table);
    const GeneSegments &S = model->host.table[table];
    const size_t n = (size_t)S.size();
    if (n && (!start || !end || !value)) return fail(BSIG_ERR_ARG, "output buffer is NULL");
    memcpy(ref_off, S.ref_off.data(), S.ref_off.size() * sizeof(int64_t));
    if (n) {
        memcpy(start, S.start.data(), n * sizeof(int32_t));
        memcpy(end, S.end.data(), n * sizeof(int32_t));
        memcpy(value, S.value.data(), n * sizeof(int32_t));
    }
    return BSIG_OK;
}

int64_t bsig_reads_n_source_reads(const bsig_reads *reads) { return reads && reads->spliced ? reads->rtab.n : 0; }

int bsig_reads_gene_counts(const bsig_reads *reads, const bsig_gene_model *model, int32_t mapqual, int32_t requiredF, int32_t filteredF,
                           int32_t strandedness, int64_t *counts, int64_t *summary)
{
    return bsig::gene_counts_query(reads, model, nullptr, mapqual, requiredF, filteredF, strandedness, counts, summary);
}

}  // extern "C"
