// Variant and mixed-allele sites (sites.hip): the cells of a nucleotide count that disagree with a reference, or among
// themselves, found on the GPU from the base table of a set with bases.  Internal: not part of the C ABI.
#ifndef BSIG_SITES_H
#define BSIG_SITES_H
#include "filecall.h"
#include "runtime_internal.h"
#include "sitemath.h"

// the host-side result: seg_off and the columns pos, alleles (4 bytes a site each) and counts (24 a site, 48 with ss), in the
// caller's range order; seconds: device time of count + scan + offsets, of the fill, and the download's
struct bsig_sites_result : bsig::EncodedColumns {
    int32_t ss = 0;
    double seconds[3] = {0, 0, 0};
};

namespace bsig {

// what a site query asks of its parameters, before anything else is looked at (the nucleotide rule included)
int sites_rule(int32_t min_base_qual, int32_t min_depth, int32_t min_alt, int32_t frac_num, int32_t frac_den, int32_t alt_mask);
// ... and of its reference codes: n_ranges widths (negative ones are left to the range rule), sum(len) codes 0 .. 4 or NULL
int sites_ref_rule(int64_t n, const int32_t *len, const uint8_t *ref);

// The query (the body of bsig_reads_sites and of the file-level call): the sites of every range, in the caller's range order
int sites_query(const bsig_reads *R, int64_t n, const int32_t *rid, const int32_t *loc, const int32_t *len, const int32_t *strand,
                int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t min_base_qual, int32_t ss, const uint8_t *ref,
                const SiteParams &prm, bsig_sites_result *out);

}  // namespace bsig
#endif
