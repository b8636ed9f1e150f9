// Reads per gene (genecounts.hip): the gene model as the C ABI holds it, and the per-read query over a spliced set's read
// table.  Internal: not part of the C ABI.
#ifndef BSIG_GENECOUNTS_H
#define BSIG_GENECOUNTS_H
#include <map>
#include <memory>
#include <mutex>

#include "genemodel.h"
#include "runtime_internal.h"

// A gene model: the three flattened tables on the host (genemodel.h) and, per GPU that has answered a query with it, their
// copy in device memory -- start, end and value of the three tables back to back, made at the first query on that GPU
struct bsig_gene_model {
    bsig::GeneModel host;
    struct OnDevice {
        DevPool pool;
        const int32_t *start = nullptr, *end = nullptr, *value = nullptr;
    };
    mutable std::mutex mu;
    mutable std::map<int, std::unique_ptr<OnDevice>> dev;
    int64_t base(int table) const       // the first segment of a table in the device columns
    {
        int64_t b = 0;
        for (int t = 0; t < table; ++t) b += host.table[t].size();
        return b;
    }
};

namespace bsig {

constexpr int kGeneSummary = 5;     // assigned, ambiguous, no_feature, filtered, unmapped

// what a gene count asks of its parameters, before anything else is looked at
int gene_counts_rule(const bsig_gene_model *model, int32_t strandedness, const int64_t *counts, const int64_t *summary);

// The query (bsig_reads_gene_counts' body): every read of R's read table classified, counts[n_genes] and summary[5] filled.
// ref_map: NULL (the set's reference r is the model's r; the model's n_ref must be the set's), or for each of the set's
// references the model's reference or -1 (the file-level call: the model's references are names).
int gene_counts_query(const bsig_reads *R, const bsig_gene_model *model, const int32_t *ref_map, int32_t mapqual, int32_t requiredF,
                      int32_t filteredF, int32_t strandedness, int64_t *counts, int64_t *summary);

}  // namespace bsig
#endif
