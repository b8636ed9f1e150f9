// Variant and mixed-allele sites (sites.hip): what is plain arithmetic -- the parameters and their rule, and the decision
// whether the six channel counts of a cell make a site.  No HIP in here: host code and sanitizer builds include it as it is;
// under hipcc site_classify is a device function as well, and the kernel calls this very function.
#ifndef BSIG_SITEMATH_H
#define BSIG_SITEMATH_H
#include <stdint.h>

#include "nucmath.h"

namespace bsig {

constexpr int32_t kSiteMaxFracDen = 1 << 20;
constexpr int32_t kSiteRefN = 4;                // a reference code that is never a site
constexpr uint32_t kSiteAllChannels = 0x3Fu;

struct SiteParams {
    int32_t min_depth, min_alt, frac_num, frac_den;
    uint32_t alt_mask;
};

// what a site query asks of its parameters: NULL, or the sentence that says what is wrong (each refusal its own)
inline const char *site_rule_sentence(int32_t min_depth, int32_t min_alt, int32_t frac_num, int32_t frac_den, int32_t alt_mask)
{
    if (min_depth < 1) return "min_depth must be at least 1";
    if (min_alt < 1) return "min_alt must be at least 1";
    if (frac_den < 1 || frac_den > kSiteMaxFracDen) return "frac_den must lie between 1 and 2^20";
    if (frac_num < 0 || frac_num > frac_den) return "frac_num must lie between 0 and frac_den";
    if (alt_mask <= 0 || alt_mask > (int32_t)kSiteAllChannels) return "alt_mask must be a nonzero mask of the six channels (bits 0 .. 5)";
    return nullptr;
}

// Is the cell with the six counts c (A C G T N '-', the strands summed) a site?  ref_code: the cell's reference channel
// 0 .. 4, or negative where the call has no reference (the base channel is then the first of the largest counts).
// -1: no site; else b | a << 8, the base and the alt channel.
BSIG_NUC_HD inline int32_t site_classify(const int64_t *c, int32_t ref_code, const SiteParams &prm)
{
    if (ref_code == kSiteRefN) return -1;
    int64_t depth = 0;
    for (int k = 0; k < kNucChannels; ++k) depth += c[k];
    if (depth < (int64_t)prm.min_depth) return -1;
    // (the running largest counts are kept as values, not looked up by a channel found at run time: the six counts stay in
    // registers on the device)
    int b = ref_code;
    if (ref_code < 0) {
        b = 0;
        int64_t cb = c[0];
        for (int k = 1; k < kNucChannels; ++k)
            if (c[k] > cb) { b = k; cb = c[k]; }
    }
    int a = -1;
    int64_t ca = -1;
    for (int k = 0; k < kNucChannels; ++k) {
        if (k == b || !((prm.alt_mask >> k) & 1u)) continue;
        if (c[k] > ca) { a = k; ca = c[k]; }
    }
    if (a < 0) return -1;           // (the mask names no channel but b)
    if (ca < (int64_t)prm.min_alt) return -1;
    if (ca * (int64_t)prm.frac_den < (int64_t)prm.frac_num * depth) return -1;
    return (int32_t)(b | (a << 8));
}

}  // namespace bsig
#endif
