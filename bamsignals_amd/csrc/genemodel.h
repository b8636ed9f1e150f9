// The gene model of bamGeneCounts: features (reference, loc, len, strand) that belong to genes, flattened into disjoint
// segment tables so that "which genes does this read touch, and is that exactly one?" needs no sets.  Plain integers and
// vectors only -- no HIP, no ABI types -- so that a host program can call it.
//
// One table per strand class: UNSTRANDED holds every feature, PLUS the features with strand +1 or 0, MINUS those with
// strand -1 or 0.  Per reference the table's features are swept from left to right: where exactly one distinct gene is
// active the stretch carries that gene, where two or more are it carries kGeneAmbig, where none is there is no segment;
// touching stretches of equal value are one segment.  A read that walks the segments its blocks touch in ONE table then
// decides: no segment -- no feature; a kGeneAmbig segment or two different values -- ambiguous; else the one value.  That
// equals the set rule (the distinct genes with a matching feature that shares a base with a block): a base's segment says
// whether the set of genes at that base is empty, one gene or larger, and the union over the bases of the blocks has one
// element iff every touched base with genes names the same single gene.
#ifndef BSIG_GENEMODEL_H
#define BSIG_GENEMODEL_H
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

namespace bsig {

constexpr int32_t kGeneAmbig = -1;          // a segment's value where two or more genes overlap
enum GeneTable { kGeneUnstranded = 0, kGenePlus = 1, kGeneMinus = 2, kGeneTables = 3 };

// one flattened table: segment k covers [start[k], end[k]] (first and last base) with value[k] (a gene or kGeneAmbig); the
// segments of reference r are ref_off[r] .. ref_off[r + 1], ascending and disjoint
struct GeneSegments {
    std::vector<int64_t> ref_off;
    std::vector<int32_t> start, end, value;
    int64_t size() const { return (int64_t)start.size(); }
};

struct GeneModel {
    int32_t n_ref = 0, n_genes = 0;
    int64_t n_features = 0;
    GeneSegments table[kGeneTables];
};

// what a model asks of its features; "" if they are fine, else the refusal in its own words, naming the first offender
inline std::string gene_model_refusal(int64_t n, const int32_t *rid, const int32_t *loc, const int32_t *len, const int32_t *strand,
                                      const int32_t *gene, int32_t n_genes, int32_t n_ref)
{
    if (n < 0 || n_genes < 0 || n_ref < 0) return "a gene model needs n, n_genes and n_ref that are not negative";
    if (n > 0 && (!rid || !loc || !len || !strand || !gene)) return "feature arrays missing";
    for (int64_t i = 0; i < n; ++i) {
        const std::string at = "feature " + std::to_string(i);
        if (len[i] < 0) return at + " has a negative width";
        if (rid[i] < 0 || rid[i] >= n_ref) return at + ": reference " + std::to_string(rid[i]) + " is not one of the model's " + std::to_string(n_ref);
        if (gene[i] < 0 || gene[i] >= n_genes) return at + ": gene " + std::to_string(gene[i]) + " is not one of the model's " + std::to_string(n_genes);
        if (strand[i] < -1 || strand[i] > 1) return at + ": strand " + std::to_string(strand[i]) + " is none of -1, 0, 1";
        if ((int64_t)loc[i] + len[i] > INT32_MAX) return at + " ends beyond base 2^31 - 1";
    }
    return std::string();
}

// does a feature of this strand enter the table?
inline bool gene_table_takes(int table, int32_t strand)
{
    return table == kGeneUnstranded || strand == 0 || (table == kGenePlus ? strand > 0 : strand < 0);
}

// The flatten of one table.  The features must have passed gene_model_refusal.  `active` is scratch of n_genes zeros and
// is left as zeros.
inline void flatten_gene_table(int table, int64_t n, const int32_t *rid, const int32_t *loc, const int32_t *len, const int32_t *strand,
                               const int32_t *gene, int32_t n_ref, std::vector<int32_t> &active, GeneSegments *out)
{
    out->ref_off.assign((size_t)n_ref + 1, 0);
    out->start.clear(); out->end.clear(); out->value.clear();
    // the table's features by reference (a counting sort: the order inside a reference does not matter to the sweep)
    std::vector<int64_t> first((size_t)n_ref + 1, 0);
    for (int64_t i = 0; i < n; ++i)
        if (len[i] > 0 && gene_table_takes(table, strand[i])) ++first[(size_t)rid[i] + 1];
    for (int32_t r = 0; r < n_ref; ++r) first[(size_t)r + 1] += first[(size_t)r];
    std::vector<int64_t> by_ref((size_t)first[(size_t)n_ref]);
    {
        std::vector<int64_t> at(first.begin(), first.end() - 1);
        for (int64_t i = 0; i < n; ++i)
            if (len[i] > 0 && gene_table_takes(table, strand[i])) by_ref[(size_t)at[(size_t)rid[i]]++] = i;
    }
    // an event: (position, gene << 1 | opens); a feature opens at loc and closes at loc + len
    std::vector<std::pair<int64_t, int64_t>> ev;
    for (int32_t r = 0; r < n_ref; ++r) {
        ev.clear();
        for (int64_t k = first[(size_t)r]; k < first[(size_t)r + 1]; ++k) {
            const int64_t i = by_ref[(size_t)k];
            ev.emplace_back((int64_t)loc[i], (int64_t)gene[i] << 1 | 1);
            ev.emplace_back((int64_t)loc[i] + len[i], (int64_t)gene[i] << 1);
        }
        std::sort(ev.begin(), ev.end());
        // distinct active genes and the sum of their ids: with one active gene the sum is that gene
        int64_t distinct = 0, id_sum = 0;
        bool open = false;
        int32_t cur = 0;
        int64_t cur_start = 0;
        for (size_t e = 0; e < ev.size();) {
            const int64_t p = ev[e].first;
            for (; e < ev.size() && ev[e].first == p; ++e) {
                const int32_t g = (int32_t)(ev[e].second >> 1);
                if (ev[e].second & 1) {
                    if (active[(size_t)g]++ == 0) { ++distinct; id_sum += g; }
                } else if (--active[(size_t)g] == 0) {
                    --distinct; id_sum -= g;
                }
            }
            const bool now_open = distinct > 0;
            const int32_t now = distinct == 1 ? (int32_t)id_sum : kGeneAmbig;
            if (open && (!now_open || now != cur)) {
                out->start.push_back((int32_t)cur_start);
                out->end.push_back((int32_t)(p - 1));
                out->value.push_back(cur);
                open = false;
            }
            if (now_open && !open) { open = true; cur = now; cur_start = p; }
        }
        out->ref_off[(size_t)r + 1] = out->size();
    }
}

// the three tables of the features; they must have passed gene_model_refusal
inline void build_gene_model(int64_t n, const int32_t *rid, const int32_t *loc, const int32_t *len, const int32_t *strand,
                             const int32_t *gene, int32_t n_genes, int32_t n_ref, GeneModel *out)
{
    out->n_ref = n_ref; out->n_genes = n_genes; out->n_features = n;
    std::vector<int32_t> active((size_t)n_genes, 0);
    for (int t = 0; t < kGeneTables; ++t) flatten_gene_table(t, n, rid, loc, len, strand, gene, n_ref, active, &out->table[t]);
}

}  // namespace bsig
#endif
