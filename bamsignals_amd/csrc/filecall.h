// What fileapi.cpp's entry points hand to the file-level dispatcher (filecall.cpp), and what the dispatcher needs of a BAM
// handle.  Internal: not part of the C ABI.
#ifndef BSIG_FILECALL_H
#define BSIG_FILECALL_H
#include <stdint.h>

#include <vector>

#include "../../include/bamsignals_abi.h"
#include "bamio.h"
#include "runtime_internal.h"

namespace bsig {

// the host-side result of an encoded file-level call, in the caller's range order: segment k owns entries seg_off[k] ..
// seg_off[k + 1] of every value column (runs: values, lengths; views: start, width, sum, max, summit)
struct EncodedColumns {
    static constexpr int kMaxCols = 5;
    int64_t n_seg = 0;
    std::vector<int64_t> seg_off;
    std::vector<uint8_t> col[kMaxCols];
    int64_t entries() const { return seg_off.empty() ? 0 : seg_off.back(); }
};
// which encoder a call's blocks go through (runs.hip / views.hip), and the bytes of an entry of each value column
enum class EncoderKind { runs, views };
struct Encoder {
    EncoderKind kind;
    const char *noun;                   // the route's word
    int n_cols;
    size_t elem[EncodedColumns::kMaxCols];
    int32_t lower = 0, upper = 0;       // views: the thresholds
};
inline Encoder runs_encoder() { return Encoder{EncoderKind::runs, "runs", 2, {4, 4, 0, 0, 0}}; }
inline Encoder views_encoder(int32_t lower, int32_t upper) { return Encoder{EncoderKind::views, "views", 5, {4, 4, 8, 4, 4}, lower, upper}; }

// Where a file-level call's result goes: one flat buffer (out, at off: bsig_layout), one vector per range (dst; bamCount's
// layout is one vector, dst[0]), one int64 vector for a reduction over the ranges, an encoder's columns, or the columns of
// a junction query (junctions.hip), the two int64 vectors of a gene count (genecounts.hip), the int32 cells of a nucleotide
// count (nucleotides.hip: bsig_nucleotides_cells' layout, not bsig_layout's), or the sites among those cells (sites.hip)
enum class Reduce { none, sum, xcorr, frag, hist, summary, scaled, vplot, capped };
struct FileDest {
    enum class Shape { flat, into, reduced, encoded, junctions, genes, nucleotides, sites } shape = Shape::flat;
    int32_t *out = nullptr;
    const int64_t *off = nullptr;
    int32_t *const *dst = nullptr;
    Reduce kind = Reduce::none;
    int64_t *reduced = nullptr;     // the kind's cells: the sum's bins, max_lag + 1 + BSIG_XCORR_MOMENTS, tlen_filter[1] / len_bin + 1
                                    // rows, max_value + 1 + BSIG_HIST_MOMENTS
    const char *name = "out";       // ... as the entry point calls that argument
    int32_t arg = 0;                // xcorr: max_lag; frag, vplot: len_bin; hist: max_value; summary: the number of thresholds; scaled: n_bins;
                                    // capped: keep_dup; junctions: min_anchor; genes: strandedness; nucleotides, sites: min_base_qual
    const int32_t *thresholds = nullptr;    // summary: arg of them
    EncodedColumns *runs = nullptr;         // the per-range result as runs or views (enc says which), in the caller's range order
    Encoder enc = runs_encoder();
    EncodedColumns *junctions = nullptr;    // the ranges' distinct junctions with their counts: start, end, count, max_anchor
    const bsig_gene_model *model = nullptr; // a gene count: the model, counts[n_genes] and summary[5]
    int64_t *gene_counts = nullptr, *gene_summary = nullptr;
    bsig_sites_result *sites = nullptr;     // the sites of the ranges' nucleotide cells: the rule's five numbers (min_depth, min_alt,
    int32_t site_rule[5] = {0, 0, 0, 0, 0}; // frac_num, frac_den, alt_mask) and the reference codes (sum(width) bytes, or NULL)
    const uint8_t *site_ref = nullptr;
    static FileDest flat(int32_t *out, const int64_t *off)
    {
        FileDest to;
        to.out = out; to.off = off;
        return to;
    }
    static FileDest into(int32_t *const *dst)
    {
        FileDest to;
        to.shape = Shape::into; to.dst = dst;
        return to;
    }
    static FileDest reduce(Reduce kind, int64_t *cells, int32_t arg = 0, const int32_t *thresholds = nullptr)
    {
        FileDest to;
        to.shape = Shape::reduced; to.kind = kind; to.reduced = cells; to.arg = arg; to.thresholds = thresholds;
        return to;
    }
    // the capped signals: a reduction plan's route, but the result is int32 cells at the caller's offsets (out, off), as a
    // plain call's -- `reduced` stays NULL
    static FileDest capped(int32_t *out, const int64_t *off, int32_t keep_dup)
    {
        FileDest to;
        to.shape = Shape::reduced; to.kind = Reduce::capped; to.out = out; to.off = off; to.arg = keep_dup;
        return to;
    }
    static FileDest encoded(EncodedColumns *cols, const Encoder &enc)
    {
        FileDest to;
        to.shape = Shape::encoded; to.runs = cols; to.enc = enc;
        return to;
    }
    static FileDest junction_table(EncodedColumns *cols, int32_t min_anchor)
    {
        FileDest to;
        to.shape = Shape::junctions; to.junctions = cols; to.arg = min_anchor;
        return to;
    }
    static FileDest nucleotide_cells(int32_t *out, int32_t min_base_qual)
    {
        FileDest to;
        to.shape = Shape::nucleotides; to.out = out; to.arg = min_base_qual;
        return to;
    }
    static FileDest site_table(bsig_sites_result *res, int32_t min_base_qual, const uint8_t *ref, int32_t min_depth, int32_t min_alt,
                               int32_t frac_num, int32_t frac_den, int32_t alt_mask)
    {
        FileDest to;
        to.shape = Shape::sites; to.sites = res; to.arg = min_base_qual; to.site_ref = ref;
        to.site_rule[0] = min_depth; to.site_rule[1] = min_alt; to.site_rule[2] = frac_num; to.site_rule[3] = frac_den; to.site_rule[4] = alt_mask;
        return to;
    }
    static FileDest gene_table(const bsig_gene_model *model, int32_t strandedness, int64_t *counts, int64_t *summary)
    {
        FileDest to;
        to.shape = Shape::genes; to.model = model; to.arg = strandedness; to.gene_counts = counts; to.gene_summary = summary;
        return to;
    }
};

// the GRanges slots as the shim flattens them: the eight arguments every file-level entry point begins with
struct RangeArgs {
    const char *bampath;
    int64_t n;
    const int32_t *seq_code;
    int32_t n_levels;
    const char *const *levels;
    const int32_t *start, *width, *strand;
};
// One file-level call.  What an entry point judges of its own before any I/O is named here and judged by the dispatcher,
// in this order: the output argument, the views' thresholds, the overlap type and its filter, the resized rule, and -- where
// rule_first says so -- the plan's parameter rule.  Every other call meets that rule after the BAM is open.
struct FileCall {
    RangeArgs at;
    bsig_params prm;
    int32_t device;
    FileDest to;
    int32_t frag_len = 0;           // a resized call (its length is judged even where it is 0)
    bool resized = false;
    bool rule_first = false;
    bool overlap = false;           // bamOverlaps: its type as given, and whether a tlen_filter was promised but not passed
    int32_t overlap_type = 0;
    bool filter_missing = false;
    bool spliced = false;           // coverage that skips N gaps, the junctions, the gene counts: the call runs on the file's spliced
                                    // reads (splice.hip)
    bool bases = false;             // the nucleotide counts and the sites: the call runs on the file's reads with bases (nucleotides.hip), a
                                    // resident set of its own
    bool whole_file = false;        // the call speaks of every read of the file (the gene counts): never an index-driven decode
};
int file_level(const FileCall &call);

// segment k of src goes to range which[k] of the destination (the body of bsig_scatter_segments; the destination may be
// one flat buffer or one vector per range)
int scatter_segments_to(int64_t n, const int32_t *src, const int64_t *src_off, const HostDest &dst, const int64_t *which);

}  // namespace bsig
struct bsig_runs_result : bsig::EncodedColumns {};
struct bsig_views_result : bsig::EncodedColumns {};
struct bsig_sites_result;       // (sites.h)

// a BAM handle as the file-level calls open it (fileapi.cpp): the header now, the index parsed by a helper thread;
// bam_index_wait joins that parse and reports what it found, bsig_bam_index joins and hands out the index
int bam_open_lazy(const char *path, bsig_bam **out);
int bam_index_wait(const bsig_bam *b);
const bsig::BaiIndex *bsig_bam_index(const bsig_bam *b);
#endif
