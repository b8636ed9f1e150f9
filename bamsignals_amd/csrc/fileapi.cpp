// File-level half of the C ABI: BAM handles, the thin file-level entry points (bsig_pileup_core / bsig_coverage_core and
// their kin: the dispatcher they call is filecall.cpp), the result handles, the BAM writers, the segment maps.  Pure host
// code; the compute goes through bsig_reads_upload / bsig_plan_*.
#include <hip/hip_runtime.h>
#include <sys/stat.h>
#include <zlib.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <future>
#include <memory>
#include <string>
#include <system_error>
#include <vector>

#include "../../include/bamsignals_abi.h"
#include "bamio.h"
#include "collect.h"
#include "filecall.h"
#include "genecounts.h"
#include "host_util.h"
#include "junctions.h"
#include "nucleotides.h"
#include "sites.h"
#include "runtime_internal.h"

using bsig::EncodedColumns;
using bsig::fail;

struct bsig_bam {
    std::string path;
    bsig::BamHeader hdr;
    bsig::BaiIndex idx;
    bool from_csi = false;      // the index was read from a .csi file (htslib's bam_index_load accepts both, ref: :207)
    bsig::HostColumns cols;
    bsig::HostBases bases;      // ... of bsig_bam_decode_bases
    std::string idx_err;
    // file-level handles: the index is parsed by a helper thread.  LAST member: its destructor waits for that
    // thread, which writes idx and idx_err above
    std::shared_future<int> idx_job;
};

namespace {
void fill_columns(const bsig_bam *b, bsig_columns *c)
{
    memset(c, 0, sizeof *c);
    c->n_reads = b->cols.size();
    c->n_ref = (int32_t)b->hdr.names.size();
    c->ref_len = b->hdr.lens.data();
    c->ref_off = b->cols.ref_off.data();
    c->pos = b->cols.pos.data();
    c->flag = b->cols.flag.data();
    c->mapq = b->cols.mapq.data();
    c->tlen = b->cols.tlen.data();
    c->end = nullptr;
    c->cigar_off = b->cols.cigar_off.data();
    c->cigar = b->cols.cigar.data();
}

// the index files htslib's bam_index_load tries (ref: src/bamsignals.cpp:207), in its order (hts_idx_load looks for a
// CSI index first -- htslib is not vendored in the reference; this is its documented search order): <bam>.csi,
// <stem>.csi, <bam>.bai, <stem>.bai
std::vector<std::pair<std::string, bool>> index_candidates(const std::string &bam)
{
    std::string stem = bam;
    if (stem.size() > 4 && stem.compare(stem.size() - 4, 4, ".bam") == 0) stem.erase(stem.size() - 4);
    std::vector<std::pair<std::string, bool>> c = {{bam + ".csi", true}};
    if (stem != bam) c.push_back({stem + ".csi", true});
    c.push_back({bam + ".bai", false});
    if (stem != bam) c.push_back({stem + ".bai", false});
    return c;
}

// parses the index of b: the FIRST candidate that exists is the index, as in htslib's search (a file of a .csi name
// that is not a CSI index fails the open there -- bam_index_load returns NULL, ref: src/bamsignals.cpp:207-210 --
// and is not passed over for an older .bai beside it); 0, or an error with its message in b->idx_err
int load_index(bsig_bam *b)
{
    for (const auto &cand : index_candidates(b->path)) {
        struct stat sb;
        if (stat(cand.first.c_str(), &sb) != 0) continue;
        const int r = cand.second ? bsig::csi_load(cand.first, b->idx) : bsig::bai_load(cand.first, b->idx);
        if (r == 0) { b->from_csi = cand.second; return 0; }
        // a damaged BAI is reported as such; a .csi that is no CSI index gets the reference's own text
        if (!cand.second && r != BSIG_ERR_NOINDEX) { b->idx_err = bsig_last_error(); return r; }
        break;
    }
    b->idx_err = "BAM indexing file is not available for file " + b->path;
    return BSIG_ERR_NOINDEX;
}

// does some index file exist?  (cheap: the file-level calls parse the index in the background and only need to
// know now whether the reference's "not available" error is due; what the first existing candidate holds is the
// parse's business, see load_index)
bool index_present(const std::string &bam)
{
    for (const auto &cand : index_candidates(bam)) {
        struct stat sb;
        if (stat(cand.first.c_str(), &sb) == 0) return true;
    }
    return false;
}

// lazy: header now, index parsed by a helper thread (the north star's 10-MB BAI takes 35 ms; a whole-file
// decode never looks at it).  bam_index_wait() joins and reports what the parse found.
int bam_open_impl(const char *path, bool lazy, bsig_bam **out)
{
    if (!path || !out) return fail(BSIG_ERR_ARG, "NULL argument to bsig_bam_open");
    *out = nullptr;
    std::unique_ptr<bsig_bam> b(new bsig_bam);
    b->path = path;
    int rc = bsig::bam_read_header(b->path, b->hdr);
    if (rc == BSIG_ERR_IO) return fail(BSIG_ERR_IO, "Fail to open BAM file %s", path);
    if (rc) return rc;
    if (lazy && index_present(b->path)) {
        bsig_bam *raw = b.get();
        try {
            b->idx_job = std::async(std::launch::async, [raw] { return load_index(raw); }).share();
        } catch (const std::system_error &) {
            lazy = false;                                  // no thread to be had: parse here
        }
    } else {
        lazy = false;
    }
    if (!lazy) {
        rc = load_index(b.get());
        if (rc) return fail(rc, "%s", b->idx_err.c_str());
    }
    *out = b.release();
    return BSIG_OK;
}
}  // namespace
int bam_open_lazy(const char *path, bsig_bam **out) { return bam_open_impl(path, true, out); }

// the parsed index of an opened BAM (joins the background parse of the file-level calls' handles)
int bam_index_wait(const bsig_bam *b)
{
    if (b->idx_job.valid()) {
        const int rc = b->idx_job.get();
        if (rc) return fail(rc, "%s", b->idx_err.c_str());
    }
    return BSIG_OK;
}
const bsig::BaiIndex *bsig_bam_index(const bsig_bam *b)
{
    if (b->idx_job.valid()) b->idx_job.wait();
    return &b->idx;
}

extern "C" {

int bsig_bam_open(const char *path, bsig_bam **out) { return bam_open_impl(path, false, out); }

void bsig_bam_close(bsig_bam *b) { delete b; }

const char *bsig_bam_path(const bsig_bam *b) { return b ? b->path.c_str() : nullptr; }

int32_t bsig_bam_n_ref(const bsig_bam *b) { return b ? (int32_t)b->hdr.names.size() : 0; }

const char *bsig_bam_ref_name(const bsig_bam *b, int32_t rid)
{
    return (b && rid >= 0 && rid < (int32_t)b->hdr.names.size()) ? b->hdr.names[(size_t)rid].c_str() : nullptr;
}

int32_t bsig_bam_ref_len(const bsig_bam *b, int32_t rid)
{
    return (b && rid >= 0 && rid < (int32_t)b->hdr.lens.size()) ? b->hdr.lens[(size_t)rid] : -1;
}

int32_t bsig_bam_name2id(const bsig_bam *b, const char *name) { return (b && name) ? b->hdr.name2id(name) : -1; }

int bsig_bam_decode(bsig_bam *b, int64_t n_regions, const int32_t *rid, const int64_t *beg,
                    const int64_t *end, int32_t threads, bsig_columns *cols)
{
    if (!b || !cols) return fail(BSIG_ERR_ARG, "NULL argument to bsig_bam_decode");
    int rc;
    bsig::BamHeader h;
    if (n_regions < 0) {
        rc = bsig::bam_decode_all(b->path, threads, h, b->cols);
    } else {
        if (n_regions > 0 && (!rid || !beg || !end)) return fail(BSIG_ERR_ARG, "region arrays missing");
        std::vector<bsig::Region> rg((size_t)n_regions);
        for (int64_t i = 0; i < n_regions; ++i) rg[(size_t)i] = bsig::Region{rid[i], beg[i], end[i]};
        rc = bam_index_wait(b);
        if (rc) return rc;
        rc = bsig::bam_decode_regions(b->path, b->idx, rg, threads, h, b->cols);
    }
    if (rc) return rc;
    fill_columns(b, cols);
    return BSIG_OK;
}

int bsig_bam_decode_bases(bsig_bam *b, int64_t n_regions, const int32_t *rid, const int64_t *beg, const int64_t *end,
                          int32_t threads, bsig_columns *cols, bsig_base_columns *bases)
{
    if (!b || !cols || !bases) return fail(BSIG_ERR_ARG, "NULL argument to bsig_bam_decode_bases");
    if (n_regions > 0 && (!rid || !beg || !end)) return fail(BSIG_ERR_ARG, "region arrays missing");
    std::vector<bsig::Region> rg((size_t)std::max<int64_t>(n_regions, 0));
    for (int64_t i = 0; i < n_regions; ++i) rg[(size_t)i] = bsig::Region{rid[i], beg[i], end[i]};
    if (n_regions >= 0)
        if (const int rc = bam_index_wait(b)) return rc;
    bsig::BamHeader h;
    const int rc = bsig::bam_decode_bases(b->path, n_regions < 0 ? nullptr : &b->idx, rg, threads, h, b->cols, b->bases);
    if (rc) return rc;
    fill_columns(b, cols);
    bases->seq_off = b->bases.seq_off.data();
    bases->seq = b->bases.seq.data();
    bases->qual = b->bases.qual.data();
    return BSIG_OK;
}

int32_t bsig_effective_cpus(void) { return (int32_t)bsig::effective_cpus(); }

void bsig_bam_decode_timing(double *t6)
{
    for (int k = 0; k < 6; ++k) t6[k] = bsig::g_decode_timing[k];
}

}  // extern "C"
namespace {
using bsig::FileCall;
using bsig::FileDest;
using bsig::Reduce;
using bsig::file_level;

// The reference's two argument lists as bsig_params.  At most two filter values are copied: check_params judges their count.
bsig_params with_filter(bsig_params p, const int32_t *tlen_filter, int32_t n_tlen_filter)
{
    p.n_tlen_filter = n_tlen_filter;
    for (int k = 0; k < std::min(n_tlen_filter, 2); ++k) p.tlen_filter[k] = tlen_filter[k];
    return p;
}
bsig_params pileup_params(const int32_t *tlen_filter, int32_t n_tlen_filter, int32_t mapqual, int32_t binsize, int32_t shift,
                          int32_t ss, int32_t requiredF, int32_t filteredF, int32_t pe_mid)
{
    bsig_params p{};
    p.mode = binsize <= 0 ? BSIG_MODE_COUNT : BSIG_MODE_PROFILE;   // ref: allocateList :148
    p.mapqual = mapqual; p.binsize = binsize; p.shift = shift; p.ss = ss;
    p.requiredF = requiredF; p.filteredF = filteredF; p.pe_mid = pe_mid;
    return with_filter(p, tlen_filter, n_tlen_filter);
}
// the per-base 5' ends the histograms, summaries and scaled regions are made of
bsig_params ends_params(const int32_t *tlen_filter, int32_t n_tlen_filter, int32_t mapqual, int32_t ss, int32_t requiredF,
                        int32_t filteredF, int32_t pe_mid)
{
    return pileup_params(tlen_filter, n_tlen_filter, mapqual, 1, 0, ss != 0, requiredF, filteredF, pe_mid != 0);
}
// ex: bins and strands (BSIG_MODE_COVERAGE_EX); without, binsize and ss are not read
bsig_params coverage_params(const int32_t *tlen_filter, int32_t n_tlen_filter, int32_t mapqual, int32_t requiredF,
                            int32_t filteredF, int32_t tspan, bool ex = false, int32_t binsize = 1, int32_t ss = 0)
{
    bsig_params p{};
    p.mode = ex ? BSIG_MODE_COVERAGE_EX : BSIG_MODE_COVERAGE;
    p.mapqual = mapqual; p.binsize = ex ? binsize : 1; p.requiredF = requiredF; p.filteredF = filteredF; p.tspan = tspan;
    p.ss = ex && ss;
    return with_filter(p, tlen_filter, n_tlen_filter);
}
// the sums call their output argument "sum"
FileDest sum_dest(int64_t *sum)
{
    FileDest to = FileDest::reduce(Reduce::sum, sum);
    to.name = "sum";
    return to;
}
// bamCoverage of reads resized to the fragment: a coverage call with frag_len in tspan's place.  The dispatcher judges the
// length and the mode (bsig::resized_rule) before it opens the BAM -- with rule_first the rest of the parameters as well --
// and hands frag_len to the resized plan creators on every route.
FileCall resized_call(const bsig::RangeArgs &at, const bsig_params &p, int32_t device, const FileDest &to, int32_t frag_len, bool rule_first)
{
    FileCall c{at, p, device, to, frag_len};
    c.resized = true;
    c.rule_first = rule_first;
    return c;
}
// bamCoverage(splice = TRUE): the binned, stranded coverage calls without tspan, on the file's spliced reads -- the same
// dispatcher, the same routes; the dispatcher judges the flag -- with rule_first the rest of the parameters as well -- before
// it opens the BAM, as for the resized calls.
FileCall spliced_call(const bsig::RangeArgs &at, const bsig_params &p, int32_t device, const FileDest &to, bool rule_first)
{
    FileCall c{at, p, device, to};
    c.spliced = true;
    c.rule_first = rule_first;
    return c;
}

// A call whose result is a host-side handle (runs, views): made here, filled by the dispatcher through the encoder `enc`,
// and the caller's only if the call succeeds.
template <typename Result>
int encoded_call(FileCall call, const bsig::Encoder &enc, Result **result)
{
    if (!result) return fail(BSIG_ERR_ARG, "result is NULL");
    *result = nullptr;
    std::unique_ptr<Result> res(new Result);
    call.to = FileDest::encoded(res.get(), enc);
    const int rc = file_level(call);
    if (rc == BSIG_OK) *result = res.release();
    return rc;
}
}  // namespace

// ---- the file-level entry points: each states its parameters and where its result goes, and makes one call ----------
extern "C" {

int bsig_pileup_core(const char *bampath, int64_t n, const int32_t *seq_code, int32_t n_levels,
                     const char *const *levels, const int32_t *start, const int32_t *width,
                     const int32_t *strand, const int32_t *tlen_filter, int32_t n_tlen_filter,
                     int32_t mapqual, int32_t binsize, int32_t shift, int32_t ss, int32_t requiredF,
                     int32_t filteredF, int32_t pe_mid, int32_t maxgap, int32_t device, int32_t *out,
                     const int64_t *off)
{
    return file_level({{bampath, n, seq_code, n_levels, levels, start, width, strand},
                       pileup_params(tlen_filter, n_tlen_filter, mapqual, binsize, shift, ss, requiredF, filteredF, pe_mid), device,
                       FileDest::flat(out, off)});
}

int bsig_pileup_core_into(const char *bampath, int64_t n, const int32_t *seq_code, int32_t n_levels,
                          const char *const *levels, const int32_t *start, const int32_t *width,
                          const int32_t *strand, const int32_t *tlen_filter, int32_t n_tlen_filter,
                          int32_t mapqual, int32_t binsize, int32_t shift, int32_t ss, int32_t requiredF,
                          int32_t filteredF, int32_t pe_mid, int32_t maxgap, int32_t device, int32_t *const *dst)
{
    return file_level({{bampath, n, seq_code, n_levels, levels, start, width, strand},
                       pileup_params(tlen_filter, n_tlen_filter, mapqual, binsize, shift, ss, requiredF, filteredF, pe_mid), device,
                       FileDest::into(dst)});
}

// bamOverlaps: a plain plan of one of the overlap modes (min_overlap in the binsize field); the type, the filter and the
// plan's rule are judged before the BAM is opened
int bsig_overlap_core(const char *bampath, int64_t n, const int32_t *seq_code, int32_t n_levels,
                      const char *const *levels, const int32_t *start, const int32_t *width,
                      const int32_t *strand, const int32_t *tlen_filter, int32_t n_tlen_filter,
                      int32_t mapqual, int32_t overlap_type, int32_t min_overlap, int32_t ss,
                      int32_t requiredF, int32_t filteredF, int32_t tspan, int32_t maxgap, int32_t device,
                      int32_t *out, const int64_t *off)
{
    bsig_params p{};
    p.mode = overlap_type ? BSIG_MODE_OVERLAP_WITHIN : BSIG_MODE_OVERLAP_ANY;
    p.mapqual = mapqual; p.binsize = min_overlap; p.ss = ss;
    p.requiredF = requiredF; p.filteredF = filteredF; p.tspan = tspan;
    const bool filter_missing = n_tlen_filter > 0 && !tlen_filter;      // (refused before anything reads the filter)
    FileCall c{{bampath, n, seq_code, n_levels, levels, start, width, strand}, with_filter(p, tlen_filter, filter_missing ? 0 : n_tlen_filter),
               device, FileDest::flat(out, off)};
    c.rule_first = c.overlap = true;
    c.overlap_type = overlap_type;
    c.filter_missing = filter_missing;
    return file_level(c);
}

int bsig_coverage_core(const char *bampath, int64_t n, const int32_t *seq_code, int32_t n_levels,
                       const char *const *levels, const int32_t *start, const int32_t *width,
                       const int32_t *strand, const int32_t *tlen_filter, int32_t n_tlen_filter,
                       int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t tspan,
                       int32_t maxgap, int32_t device, int32_t *out, const int64_t *off)
{
    return file_level({{bampath, n, seq_code, n_levels, levels, start, width, strand},
                       coverage_params(tlen_filter, n_tlen_filter, mapqual, requiredF, filteredF, tspan), device, FileDest::flat(out, off)});
}

int bsig_coverage_core_into(const char *bampath, int64_t n, const int32_t *seq_code, int32_t n_levels,
                            const char *const *levels, const int32_t *start, const int32_t *width,
                            const int32_t *strand, const int32_t *tlen_filter, int32_t n_tlen_filter,
                            int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t tspan,
                            int32_t maxgap, int32_t device, int32_t *const *dst)
{
    return file_level({{bampath, n, seq_code, n_levels, levels, start, width, strand},
                       coverage_params(tlen_filter, n_tlen_filter, mapqual, requiredF, filteredF, tspan), device, FileDest::into(dst)});
}

int bsig_coverage_core_ex(const char *bampath, int64_t n, const int32_t *seq_code, int32_t n_levels,
                          const char *const *levels, const int32_t *start, const int32_t *width,
                          const int32_t *strand, const int32_t *tlen_filter, int32_t n_tlen_filter,
                          int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t tspan,
                          int32_t maxgap, int32_t device, int32_t binsize, int32_t ss, int32_t *out, const int64_t *off)
{
    return file_level({{bampath, n, seq_code, n_levels, levels, start, width, strand},
                       coverage_params(tlen_filter, n_tlen_filter, mapqual, requiredF, filteredF, tspan, true, binsize, ss), device,
                       FileDest::flat(out, off)});
}

int bsig_coverage_core_ex_into(const char *bampath, int64_t n, const int32_t *seq_code, int32_t n_levels,
                               const char *const *levels, const int32_t *start, const int32_t *width,
                               const int32_t *strand, const int32_t *tlen_filter, int32_t n_tlen_filter,
                               int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t tspan,
                               int32_t maxgap, int32_t device, int32_t binsize, int32_t ss, int32_t *const *dst)
{
    return file_level({{bampath, n, seq_code, n_levels, levels, start, width, strand},
                       coverage_params(tlen_filter, n_tlen_filter, mapqual, requiredF, filteredF, tspan, true, binsize, ss), device,
                       FileDest::into(dst)});
}

int bsig_pileup_sum(const char *bampath, int64_t n, const int32_t *seq_code, int32_t n_levels,
                    const char *const *levels, const int32_t *start, const int32_t *width,
                    const int32_t *strand, const int32_t *tlen_filter, int32_t n_tlen_filter,
                    int32_t mapqual, int32_t binsize, int32_t shift, int32_t ss, int32_t requiredF,
                    int32_t filteredF, int32_t pe_mid, int32_t maxgap, int32_t device, int64_t *sum)
{
    return file_level({{bampath, n, seq_code, n_levels, levels, start, width, strand},
                       pileup_params(tlen_filter, n_tlen_filter, mapqual, binsize, shift, ss, requiredF, filteredF, pe_mid), device,
                       sum_dest(sum)});
}

int bsig_coverage_sum(const char *bampath, int64_t n, const int32_t *seq_code, int32_t n_levels,
                      const char *const *levels, const int32_t *start, const int32_t *width,
                      const int32_t *strand, const int32_t *tlen_filter, int32_t n_tlen_filter,
                      int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t tspan,
                      int32_t maxgap, int32_t device, int32_t binsize, int32_t ss, int64_t *sum)
{
    return file_level({{bampath, n, seq_code, n_levels, levels, start, width, strand},
                       coverage_params(tlen_filter, n_tlen_filter, mapqual, requiredF, filteredF, tspan, true, binsize, ss), device,
                       sum_dest(sum)});
}

int bsig_pileup_xcorr(const char *bampath, int64_t n, const int32_t *seq_code, int32_t n_levels,
                      const char *const *levels, const int32_t *start, const int32_t *width,
                      const int32_t *strand, const int32_t *tlen_filter, int32_t n_tlen_filter,
                      int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t max_lag, int32_t maxgap,
                      int32_t device, int64_t *out)
{
    return file_level({{bampath, n, seq_code, n_levels, levels, start, width, strand},
                       pileup_params(tlen_filter, n_tlen_filter, mapqual, 1, 0, 1, requiredF, filteredF, 0), device,
                       FileDest::reduce(Reduce::xcorr, out, max_lag)});
}

int bsig_pileup_frag(const char *bampath, int64_t n, const int32_t *seq_code, int32_t n_levels,
                     const char *const *levels, const int32_t *start, const int32_t *width,
                     const int32_t *strand, const int32_t *tlen_filter, int32_t n_tlen_filter,
                     int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t pe_mid, int32_t len_bin, int32_t maxgap,
                     int32_t device, int64_t *out)
{
    return file_level({{bampath, n, seq_code, n_levels, levels, start, width, strand},
                       pileup_params(tlen_filter, n_tlen_filter, mapqual, -1, 0, 0, requiredF, filteredF, pe_mid != 0), device,
                       FileDest::reduce(Reduce::frag, out, len_bin)});
}

int bsig_pileup_vplot(const char *bampath, int64_t n, const int32_t *seq_code, int32_t n_levels,
                      const char *const *levels, const int32_t *start, const int32_t *width,
                      const int32_t *strand, const int32_t *tlen_filter, int32_t n_tlen_filter,
                      int32_t mapqual, int32_t binsize, int32_t requiredF, int32_t filteredF, int32_t pe_mid, int32_t len_bin,
                      int32_t maxgap, int32_t device, int64_t *out)
{
    bsig_params p = pileup_params(tlen_filter, n_tlen_filter, mapqual, 1, 0, 0, requiredF, filteredF, pe_mid != 0);
    p.binsize = binsize;        // (the position bin travels here; vplot_shape judges it: below 1 it is no bamCount)
    return file_level({{bampath, n, seq_code, n_levels, levels, start, width, strand}, p, device,
                       FileDest::reduce(Reduce::vplot, out, len_bin)});
}

int bsig_pileup_hist(const char *bampath, int64_t n, const int32_t *seq_code, int32_t n_levels,
                     const char *const *levels, const int32_t *start, const int32_t *width,
                     const int32_t *strand, const int32_t *tlen_filter, int32_t n_tlen_filter,
                     int32_t mapqual, int32_t ss, int32_t requiredF, int32_t filteredF, int32_t pe_mid, int32_t max_value,
                     int32_t maxgap, int32_t device, int64_t *out)
{
    return file_level({{bampath, n, seq_code, n_levels, levels, start, width, strand},
                       ends_params(tlen_filter, n_tlen_filter, mapqual, ss, requiredF, filteredF, pe_mid), device,
                       FileDest::reduce(Reduce::hist, out, max_value)});
}

int bsig_coverage_hist(const char *bampath, int64_t n, const int32_t *seq_code, int32_t n_levels,
                       const char *const *levels, const int32_t *start, const int32_t *width,
                       const int32_t *strand, const int32_t *tlen_filter, int32_t n_tlen_filter,
                       int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t tspan, int32_t max_value,
                       int32_t maxgap, int32_t device, int64_t *out)
{
    return file_level({{bampath, n, seq_code, n_levels, levels, start, width, strand},
                       coverage_params(tlen_filter, n_tlen_filter, mapqual, requiredF, filteredF, tspan), device,
                       FileDest::reduce(Reduce::hist, out, max_value)});
}

int bsig_pileup_summary(const char *bampath, int64_t n, const int32_t *seq_code, int32_t n_levels,
                        const char *const *levels, const int32_t *start, const int32_t *width,
                        const int32_t *strand, const int32_t *tlen_filter, int32_t n_tlen_filter,
                        int32_t mapqual, int32_t ss, int32_t requiredF, int32_t filteredF, int32_t pe_mid,
                        int32_t n_thresholds, const int32_t *thresholds, int32_t maxgap, int32_t device, int64_t *out)
{
    return file_level({{bampath, n, seq_code, n_levels, levels, start, width, strand},
                       ends_params(tlen_filter, n_tlen_filter, mapqual, ss, requiredF, filteredF, pe_mid), device,
                       FileDest::reduce(Reduce::summary, out, n_thresholds, thresholds)});
}

int bsig_coverage_summary(const char *bampath, int64_t n, const int32_t *seq_code, int32_t n_levels,
                          const char *const *levels, const int32_t *start, const int32_t *width,
                          const int32_t *strand, const int32_t *tlen_filter, int32_t n_tlen_filter,
                          int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t tspan,
                          int32_t n_thresholds, const int32_t *thresholds, int32_t maxgap, int32_t device, int64_t *out)
{
    return file_level({{bampath, n, seq_code, n_levels, levels, start, width, strand},
                       coverage_params(tlen_filter, n_tlen_filter, mapqual, requiredF, filteredF, tspan), device,
                       FileDest::reduce(Reduce::summary, out, n_thresholds, thresholds)});
}

int bsig_pileup_scaled(const char *bampath, int64_t n, const int32_t *seq_code, int32_t n_levels,
                       const char *const *levels, const int32_t *start, const int32_t *width,
                       const int32_t *strand, const int32_t *tlen_filter, int32_t n_tlen_filter,
                       int32_t mapqual, int32_t ss, int32_t requiredF, int32_t filteredF, int32_t pe_mid,
                       int32_t n_bins, int32_t maxgap, int32_t device, int64_t *out)
{
    return file_level({{bampath, n, seq_code, n_levels, levels, start, width, strand},
                       ends_params(tlen_filter, n_tlen_filter, mapqual, ss, requiredF, filteredF, pe_mid), device,
                       FileDest::reduce(Reduce::scaled, out, n_bins)});
}

int bsig_coverage_scaled(const char *bampath, int64_t n, const int32_t *seq_code, int32_t n_levels,
                         const char *const *levels, const int32_t *start, const int32_t *width,
                         const int32_t *strand, const int32_t *tlen_filter, int32_t n_tlen_filter,
                         int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t tspan,
                         int32_t n_bins, int32_t maxgap, int32_t device, int64_t *out)
{
    return file_level({{bampath, n, seq_code, n_levels, levels, start, width, strand},
                       coverage_params(tlen_filter, n_tlen_filter, mapqual, requiredF, filteredF, tspan), device,
                       FileDest::reduce(Reduce::scaled, out, n_bins)});
}

int bsig_pileup_capped(const char *bampath, int64_t n, const int32_t *seq_code, int32_t n_levels,
                       const char *const *levels, const int32_t *start, const int32_t *width,
                       const int32_t *strand, const int32_t *tlen_filter, int32_t n_tlen_filter,
                       int32_t mapqual, int32_t binsize, int32_t shift, int32_t ss, int32_t requiredF, int32_t filteredF, int32_t pe_mid,
                       int32_t keep_dup, int32_t maxgap, int32_t device, int32_t *out, const int64_t *off)
{
    return file_level({{bampath, n, seq_code, n_levels, levels, start, width, strand},
                       pileup_params(tlen_filter, n_tlen_filter, mapqual, binsize, shift, ss, requiredF, filteredF, pe_mid), device,
                       FileDest::capped(out, off, keep_dup)});
}

int bsig_coverage_capped(const char *bampath, int64_t n, const int32_t *seq_code, int32_t n_levels,
                         const char *const *levels, const int32_t *start, const int32_t *width,
                         const int32_t *strand, const int32_t *tlen_filter, int32_t n_tlen_filter,
                         int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t tspan, int32_t frag_len,
                         int32_t keep_dup, int32_t maxgap, int32_t device, int32_t binsize, int32_t ss, int32_t *out,
                         const int64_t *off)
{
    FileCall c{{bampath, n, seq_code, n_levels, levels, start, width, strand},
               coverage_params(tlen_filter, n_tlen_filter, mapqual, requiredF, filteredF, tspan, true, binsize, ss), device,
               FileDest::capped(out, off, keep_dup), frag_len};
    return file_level(c);
}

int bsig_pileup_runs(const char *bampath, int64_t n, const int32_t *seq_code, int32_t n_levels,
                     const char *const *levels, const int32_t *start, const int32_t *width,
                     const int32_t *strand, const int32_t *tlen_filter, int32_t n_tlen_filter,
                     int32_t mapqual, int32_t binsize, int32_t shift, int32_t ss, int32_t requiredF,
                     int32_t filteredF, int32_t pe_mid, int32_t maxgap, int32_t device, bsig_runs_result **result)
{
    return encoded_call({{bampath, n, seq_code, n_levels, levels, start, width, strand},
                         pileup_params(tlen_filter, n_tlen_filter, mapqual, binsize, shift, ss, requiredF, filteredF, pe_mid), device, {}},
                        bsig::runs_encoder(), result);
}

int bsig_coverage_runs(const char *bampath, int64_t n, const int32_t *seq_code, int32_t n_levels,
                       const char *const *levels, const int32_t *start, const int32_t *width,
                       const int32_t *strand, const int32_t *tlen_filter, int32_t n_tlen_filter,
                       int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t tspan,
                       int32_t maxgap, int32_t device, int32_t binsize, int32_t ss, bsig_runs_result **result)
{
    return encoded_call({{bampath, n, seq_code, n_levels, levels, start, width, strand},
                         coverage_params(tlen_filter, n_tlen_filter, mapqual, requiredF, filteredF, tspan, true, binsize, ss), device, {}},
                        bsig::runs_encoder(), result);
}

int bsig_coverage_core_resized(const char *bampath, int64_t n, const int32_t *seq_code, int32_t n_levels,
                               const char *const *levels, const int32_t *start, const int32_t *width,
                               const int32_t *strand, const int32_t *tlen_filter, int32_t n_tlen_filter,
                               int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t frag_len,
                               int32_t maxgap, int32_t device, int32_t binsize, int32_t ss, int32_t *out, const int64_t *off)
{
    return file_level(resized_call({bampath, n, seq_code, n_levels, levels, start, width, strand},
                                   coverage_params(tlen_filter, n_tlen_filter, mapqual, requiredF, filteredF, 0, true, binsize, ss), device,
                                   FileDest::flat(out, off), frag_len, true));
}

int bsig_coverage_sum_resized(const char *bampath, int64_t n, const int32_t *seq_code, int32_t n_levels,
                              const char *const *levels, const int32_t *start, const int32_t *width,
                              const int32_t *strand, const int32_t *tlen_filter, int32_t n_tlen_filter,
                              int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t frag_len,
                              int32_t maxgap, int32_t device, int32_t binsize, int32_t ss, int64_t *sum)
{
    return file_level(resized_call({bampath, n, seq_code, n_levels, levels, start, width, strand},
                                   coverage_params(tlen_filter, n_tlen_filter, mapqual, requiredF, filteredF, 0, true, binsize, ss), device,
                                   sum_dest(sum), frag_len, true));
}

int bsig_coverage_runs_resized(const char *bampath, int64_t n, const int32_t *seq_code, int32_t n_levels,
                               const char *const *levels, const int32_t *start, const int32_t *width,
                               const int32_t *strand, const int32_t *tlen_filter, int32_t n_tlen_filter,
                               int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t frag_len,
                               int32_t maxgap, int32_t device, int32_t binsize, int32_t ss, bsig_runs_result **result)
{
    return encoded_call(resized_call({bampath, n, seq_code, n_levels, levels, start, width, strand},
                                     coverage_params(tlen_filter, n_tlen_filter, mapqual, requiredF, filteredF, 0, true, binsize, ss), device,
                                     {}, frag_len, false),
                        bsig::runs_encoder(), result);
}

// The three runs calls with the thresholds of the views behind their arguments: the same dispatcher, the same route, the
// views encoder in the blocks' loop.
int bsig_pileup_views(const char *bampath, int64_t n, const int32_t *seq_code, int32_t n_levels,
                      const char *const *levels, const int32_t *start, const int32_t *width,
                      const int32_t *strand, const int32_t *tlen_filter, int32_t n_tlen_filter,
                      int32_t mapqual, int32_t binsize, int32_t shift, int32_t ss, int32_t requiredF,
                      int32_t filteredF, int32_t pe_mid, int32_t maxgap, int32_t device, int32_t lower, int32_t upper,
                      bsig_views_result **result)
{
    return encoded_call({{bampath, n, seq_code, n_levels, levels, start, width, strand},
                         pileup_params(tlen_filter, n_tlen_filter, mapqual, binsize, shift, ss, requiredF, filteredF, pe_mid), device, {}},
                        bsig::views_encoder(lower, upper), result);
}

int bsig_coverage_views(const char *bampath, int64_t n, const int32_t *seq_code, int32_t n_levels,
                        const char *const *levels, const int32_t *start, const int32_t *width,
                        const int32_t *strand, const int32_t *tlen_filter, int32_t n_tlen_filter,
                        int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t tspan,
                        int32_t maxgap, int32_t device, int32_t binsize, int32_t ss, int32_t lower, int32_t upper,
                        bsig_views_result **result)
{
    return encoded_call({{bampath, n, seq_code, n_levels, levels, start, width, strand},
                         coverage_params(tlen_filter, n_tlen_filter, mapqual, requiredF, filteredF, tspan, true, binsize, ss), device, {}},
                        bsig::views_encoder(lower, upper), result);
}

int bsig_coverage_views_resized(const char *bampath, int64_t n, const int32_t *seq_code, int32_t n_levels,
                                const char *const *levels, const int32_t *start, const int32_t *width,
                                const int32_t *strand, const int32_t *tlen_filter, int32_t n_tlen_filter,
                                int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t frag_len,
                                int32_t maxgap, int32_t device, int32_t binsize, int32_t ss, int32_t lower, int32_t upper,
                                bsig_views_result **result)
{
    return encoded_call(resized_call({bampath, n, seq_code, n_levels, levels, start, width, strand},
                                     coverage_params(tlen_filter, n_tlen_filter, mapqual, requiredF, filteredF, 0, true, binsize, ss), device,
                                     {}, frag_len, false),
                        bsig::views_encoder(lower, upper), result);
}

int bsig_coverage_core_spliced(const char *bampath, int64_t n, const int32_t *seq_code, int32_t n_levels,
                               const char *const *levels, const int32_t *start, const int32_t *width,
                               const int32_t *strand, const int32_t *tlen_filter, int32_t n_tlen_filter,
                               int32_t mapqual, int32_t requiredF, int32_t filteredF,
                               int32_t maxgap, int32_t device, int32_t binsize, int32_t ss, int32_t *out, const int64_t *off)
{
    return file_level(spliced_call({bampath, n, seq_code, n_levels, levels, start, width, strand},
                                   coverage_params(tlen_filter, n_tlen_filter, mapqual, requiredF, filteredF, 0, true, binsize, ss), device,
                                   FileDest::flat(out, off), true));
}

int bsig_coverage_sum_spliced(const char *bampath, int64_t n, const int32_t *seq_code, int32_t n_levels,
                              const char *const *levels, const int32_t *start, const int32_t *width,
                              const int32_t *strand, const int32_t *tlen_filter, int32_t n_tlen_filter,
                              int32_t mapqual, int32_t requiredF, int32_t filteredF,
                              int32_t maxgap, int32_t device, int32_t binsize, int32_t ss, int64_t *sum)
{
    return file_level(spliced_call({bampath, n, seq_code, n_levels, levels, start, width, strand},
                                   coverage_params(tlen_filter, n_tlen_filter, mapqual, requiredF, filteredF, 0, true, binsize, ss), device,
                                   sum_dest(sum), true));
}

int bsig_coverage_runs_spliced(const char *bampath, int64_t n, const int32_t *seq_code, int32_t n_levels,
                               const char *const *levels, const int32_t *start, const int32_t *width,
                               const int32_t *strand, const int32_t *tlen_filter, int32_t n_tlen_filter,
                               int32_t mapqual, int32_t requiredF, int32_t filteredF,
                               int32_t maxgap, int32_t device, int32_t binsize, int32_t ss, bsig_runs_result **result)
{
    return encoded_call(spliced_call({bampath, n, seq_code, n_levels, levels, start, width, strand},
                                     coverage_params(tlen_filter, n_tlen_filter, mapqual, requiredF, filteredF, 0, true, binsize, ss), device,
                                     {}, false),
                        bsig::runs_encoder(), result);
}

int bsig_coverage_views_spliced(const char *bampath, int64_t n, const int32_t *seq_code, int32_t n_levels,
                                const char *const *levels, const int32_t *start, const int32_t *width,
                                const int32_t *strand, const int32_t *tlen_filter, int32_t n_tlen_filter,
                                int32_t mapqual, int32_t requiredF, int32_t filteredF,
                                int32_t maxgap, int32_t device, int32_t binsize, int32_t ss, int32_t lower, int32_t upper,
                                bsig_views_result **result)
{
    return encoded_call(spliced_call({bampath, n, seq_code, n_levels, levels, start, width, strand},
                                     coverage_params(tlen_filter, n_tlen_filter, mapqual, requiredF, filteredF, 0, true, binsize, ss), device,
                                     {}, false),
                        bsig::views_encoder(lower, upper), result);
}

// bamJunctions: the junctions of the ranges from the file's spliced reads.  A spliced call with a coverage call's parameters
// (the dispatcher's stages judge and decode as for bamCoverage(splice = TRUE): the same resident set) and a destination of
// its own; min_anchor is judged with the rest before the BAM is opened
int bsig_junctions(const char *bampath, int64_t n, const int32_t *seq_code, int32_t n_levels,
                   const char *const *levels, const int32_t *start, const int32_t *width,
                   const int32_t *strand, int32_t mapqual, int32_t requiredF, int32_t filteredF,
                   int32_t min_anchor, int32_t ss, int32_t device, bsig_junctions_result **result)
{
    if (!result) return fail(BSIG_ERR_ARG, "result is NULL");
    *result = nullptr;
    std::unique_ptr<bsig_junctions_result> res(new bsig_junctions_result);
    res->ss = ss != 0;
    const int rc = file_level(spliced_call({bampath, n, seq_code, n_levels, levels, start, width, strand},
                                           coverage_params(nullptr, 0, mapqual, requiredF, filteredF, 0, true, 1, ss), device,
                                           FileDest::junction_table(res.get(), min_anchor), true));
    if (rc == BSIG_OK) *result = res.release();
    return rc;
}

// bamNucleotides: A / C / G / T / N / deletion counts per base from the file's reads with bases.  The call carries a coverage
// call's parameters (the range rule is theirs: widths that are not negative); min_base_qual is judged before the BAM is opened.
int bsig_nucleotides(const char *bampath, int64_t n, const int32_t *seq_code, int32_t n_levels,
                     const char *const *levels, const int32_t *start, const int32_t *width, const int32_t *strand,
                     int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t min_base_qual, int32_t ss, int32_t device,
                     int32_t *out)
{
    bsig_params p = coverage_params(nullptr, 0, mapqual, requiredF, filteredF, 0, true, 1, ss != 0);
    FileCall c{{bampath, n, seq_code, n_levels, levels, start, width, strand}, p, device, FileDest::nucleotide_cells(out, min_base_qual)};
    c.bases = true;
    c.rule_first = true;
    return file_level(c);
}

// bamSites: the variant and mixed-allele sites among the nucleotide cells of the ranges.  bsig_nucleotides' call -- the same
// parameters, the same resident set -- with a destination of its own; the site rule and the reference codes are judged with the
// rest before the BAM is opened
int bsig_sites(const char *bampath, int64_t n, const int32_t *seq_code, int32_t n_levels,
               const char *const *levels, const int32_t *start, const int32_t *width, const int32_t *strand,
               int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t min_base_qual, int32_t ss, const uint8_t *ref,
               int32_t min_depth, int32_t min_alt, int32_t frac_num, int32_t frac_den, int32_t alt_mask, int32_t device,
               bsig_sites_result **result)
{
    if (!result) return fail(BSIG_ERR_ARG, "result is NULL");
    *result = nullptr;
    std::unique_ptr<bsig_sites_result> res(new bsig_sites_result);
    bsig_params p = coverage_params(nullptr, 0, mapqual, requiredF, filteredF, 0, true, 1, ss != 0);
    FileCall c{{bampath, n, seq_code, n_levels, levels, start, width, strand}, p, device,
               FileDest::site_table(res.get(), min_base_qual, ref, min_depth, min_alt, frac_num, frac_den, alt_mask)};
    c.bases = true;
    c.rule_first = true;
    const int rc = file_level(c);
    if (rc == BSIG_OK) *result = res.release();
    return rc;
}

// bamGeneCounts: every read of the file's spliced reads against a gene model.  A spliced call without ranges (the model's
// references are the names in seq_levels) on the whole file's resident set, with a destination of its own; the parameters are
// judged before the BAM is opened
int bsig_gene_counts(const char *bampath, const bsig_gene_model *model, int32_t n_levels, const char *const *levels, int32_t mapqual,
                     int32_t requiredF, int32_t filteredF, int32_t strandedness, int32_t device, int64_t *counts, int64_t *summary)
{
    FileCall c = spliced_call({bampath, 0, nullptr, n_levels, levels, nullptr, nullptr, nullptr},
                              coverage_params(nullptr, 0, mapqual, requiredF, filteredF, 0, true, 1, 0), device,
                              FileDest::gene_table(model, strandedness, counts, summary), true);
    c.whole_file = true;
    return file_level(c);
}

int64_t bsig_runs_result_n_seg(const bsig_runs_result *r) { return r ? r->n_seg : 0; }

int64_t bsig_runs_result_n_runs(const bsig_runs_result *r) { return r ? r->entries() : 0; }

int bsig_runs_result_copy(const bsig_runs_result *r, int64_t *seg_off, int32_t *values, int32_t *lengths)
{
    if (!r || !seg_off) return fail(BSIG_ERR_ARG, "NULL argument");
    const size_t n_runs = (size_t)r->entries();
    if (n_runs && (!values || !lengths)) return fail(BSIG_ERR_ARG, "output buffer is NULL");
    memcpy(seg_off, r->seg_off.data(), r->seg_off.size() * sizeof(int64_t));
    if (n_runs) {
        memcpy(values, r->col[0].data(), n_runs * sizeof(int32_t));
        memcpy(lengths, r->col[1].data(), n_runs * sizeof(int32_t));
    }
    return BSIG_OK;
}

void bsig_runs_result_free(bsig_runs_result *r) { delete r; }

int64_t bsig_views_result_n_seg(const bsig_views_result *r) { return r ? r->n_seg : 0; }

int64_t bsig_views_result_n_views(const bsig_views_result *r) { return r ? r->entries() : 0; }

int bsig_views_result_copy(const bsig_views_result *r, int64_t *seg_off, int32_t *start, int32_t *width, int64_t *sum, int32_t *max,
                           int32_t *summit)
{
    if (!r || !seg_off) return fail(BSIG_ERR_ARG, "NULL argument");
    const size_t n = (size_t)r->entries();
    if (n && (!start || !width || !sum || !max || !summit)) return fail(BSIG_ERR_ARG, "output buffer is NULL");
    memcpy(seg_off, r->seg_off.data(), r->seg_off.size() * sizeof(int64_t));
    void *const dst[EncodedColumns::kMaxCols] = {start, width, sum, max, summit};
    for (int c = 0; n && c < EncodedColumns::kMaxCols; ++c) memcpy(dst[c], r->col[c].data(), r->col[c].size());
    return BSIG_OK;
}

void bsig_views_result_free(bsig_views_result *r) { delete r; }

int bsig_write_sam_as_bam_and_index(const char *sampath, const char *bampath)
{
    if (!sampath || !bampath) return fail(BSIG_ERR_ARG, "NULL path");
    return bsig::sam_to_bam_and_index(sampath, bampath);
}

static int write_columns_impl(const char *bampath, int32_t n_ref, const char *const *ref_names, const bsig_columns *c,
                              int32_t level, int32_t l_seq, uint64_t seed);

int bsig_write_columns_as_bam(const char *bampath, int32_t n_ref, const char *const *ref_names,
                              const bsig_columns *c, int32_t level)
{
    return write_columns_impl(bampath, n_ref, ref_names, c, level, 0, 0);
}

int bsig_write_columns_as_bam_with_seq(const char *bampath, int32_t n_ref, const char *const *ref_names,
                                       const bsig_columns *c, int32_t level, int32_t l_seq, uint64_t seed)
{
    if (l_seq <= 0) return fail(BSIG_ERR_ARG, "l_seq must be positive");
    return write_columns_impl(bampath, n_ref, ref_names, c, level, l_seq, seed);
}

static int write_columns_impl(const char *bampath, int32_t n_ref, const char *const *ref_names, const bsig_columns *c,
                              int32_t level, int32_t l_seq, uint64_t seed)
{
    if (!bampath || !c || (n_ref > 0 && !ref_names)) return fail(BSIG_ERR_ARG, "NULL argument");
    if (c->n_ref != n_ref) return fail(BSIG_ERR_ARG, "n_ref does not match the columns");
    if (c->n_reads > 0 && (!c->cigar_off || !c->cigar)) return fail(BSIG_ERR_ARG, "the writer needs cigar_off + cigar");
    bsig::BamHeader h;
    h.text = "@HD\tVN:1.0\tSO:coordinate\n";
    for (int r = 0; r < n_ref; ++r) {
        h.names.emplace_back(ref_names[r]);
        h.lens.push_back(c->ref_len[r]);
        h.text += "@SQ\tSN:" + h.names.back() + "\tLN:" + std::to_string(c->ref_len[r]) + "\n";
    }
    bsig::BamWriter w;
    int rc = w.open(bampath, h, level > 0 ? level : 1);
    if (rc) return rc;
    const char *how = getenv("BAMSIGNALS_WRITER");      // "serial": record by record (testing)
    if (how && !strcmp(how, "serial") && !l_seq) {
        for (int r = 0; r < n_ref; ++r)
            for (int64_t i = c->ref_off[r]; i < c->ref_off[r + 1]; ++i) {
                rc = w.write_core(r, c->pos[i], c->flag[i], c->mapq[i], c->tlen[i], c->cigar + c->cigar_off[i],
                                  (int)(c->cigar_off[i + 1] - c->cigar_off[i]));
                if (rc) return rc;
            }
    } else {
        rc = w.write_columns(n_ref, c->ref_off, c->pos, c->flag, c->mapq, c->tlen, c->cigar_off, c->cigar, 0, l_seq, seed);
        if (rc) return rc;
    }
    return w.close();
}

// checkList / fastWidth (ref: src/CountSignals.cpp:4-29)
int32_t bsig_check_list(int64_t n, const int32_t *is_int, const int32_t *n_dim, const int32_t *dim0, int32_t ss)
{
    if (n > 0 && (!is_int || (ss && (!n_dim || !dim0)))) return 0;
    for (int64_t i = 0; i < n; ++i) {
        if (!is_int[i]) return 0;                                   // ref: :8
        if (ss && (n_dim[i] != 2 || dim0[i] != 2)) return 0;        // ref: :11-12
    }
    return 1;
}

void bsig_fast_width(int64_t n, const int64_t *length, int32_t ss, int32_t *width)
{
    const int64_t div = ss ? 2 : 1;                                 // ref: :21
    for (int64_t i = 0; i < n; ++i) width[i] = (int32_t)(length[i] / div);
}

int bsig_scatter_segments(int64_t n, const int32_t *src, const int64_t *src_off, int32_t *dst,
                          const int64_t *dst_off, const int64_t *which)
{
    bsig::HostDest D;
    D.flat = dst; D.off = dst_off; D.n = 0;
    return bsig::scatter_segments_to(n, src, src_off, D, which);
}

struct bsig_segmap {
    bsig_ctx *ctx = nullptr;
    int64_t n = 0;
    int64_t *d_src_off = nullptr, *d_dst_off = nullptr, *d_which = nullptr;
    int *d_overflow = nullptr;      // set by a narrow run whose sender had more exceptions than its list holds
    int64_t src_cells = 0;          // src_off[n]: a narrow message must code at least this many cells
};

int bsig_segmap_create(bsig_ctx *ctx, int64_t n, const int64_t *src_off, int64_t n_dst, const int64_t *dst_off,
                       const int64_t *which, bsig_segmap **out)
{
    if (!ctx || !out) return fail(BSIG_ERR_ARG, "NULL argument to bsig_segmap_create");
    *out = nullptr;
    if (n < 0 || n_dst < 0 || (n > 0 && (!src_off || !dst_off || !which))) return fail(BSIG_ERR_ARG, "segment tables missing");
    for (int64_t k = 0; k < n; ++k) {
        const int64_t len = src_off[k + 1] - src_off[k];
        const int64_t i = which[k];
        if (len < 0 || src_off[k] < 0 || i < 0 || i >= n_dst) return fail(BSIG_ERR_ARG, "bad segment %lld", (long long)k);
        if (dst_off[i] < 0 || len != dst_off[i + 1] - dst_off[i]) return fail(BSIG_ERR_ARG, "segment %lld does not fit its destination", (long long)k);
    }
    std::unique_ptr<bsig_segmap> M(new bsig_segmap);
    M->ctx = ctx;
    M->n = n;
    M->src_cells = n ? src_off[n] : 0;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    hipError_t e = hipMalloc((void **)&M->d_src_off, (size_t)(n + 1) * sizeof(int64_t));
    if (e == hipSuccess) e = hipMalloc((void **)&M->d_dst_off, (size_t)(n_dst + 1) * sizeof(int64_t));
    if (e == hipSuccess) e = hipMalloc((void **)&M->d_which, (size_t)std::max<int64_t>(n, 1) * sizeof(int64_t));
    if (e == hipSuccess) e = hipMalloc((void **)&M->d_overflow, sizeof(int));
    if (e == hipSuccess) e = hipMemsetAsync(M->d_overflow, 0, sizeof(int), st);
    const int64_t zero = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(M->d_src_off, n ? src_off : &zero, (size_t)(n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(M->d_dst_off, dst_off ? dst_off : &zero, (size_t)(n_dst + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && n) e = hipMemcpyAsync(M->d_which, which, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        bsig_segmap_free(M.release());
        return fail(e == hipErrorOutOfMemory ? BSIG_ERR_NOMEM : BSIG_ERR_DEVICE, "segment map upload failed: %s", hipGetErrorString(e));
    }
    *out = M.release();
    return BSIG_OK;
}

int bsig_segmap_run(bsig_segmap *M, const int32_t *src_dev, int32_t *dst_dev)
{
    if (!M) return fail(BSIG_ERR_ARG, "segment map is NULL");
    if (M->n == 0) return BSIG_OK;
    if (!src_dev || !dst_dev) return fail(BSIG_ERR_ARG, "NULL device buffer");
    HIP_TRY(hipSetDevice(M->ctx->device));
    HIP_TRY(bsig::launch_place_segments(M->n, src_dev, M->d_src_off, dst_dev, M->d_dst_off, M->d_which, M->ctx->stream));
    return BSIG_OK;
}

int64_t bsig_narrow_bytes(int64_t n_cells, int64_t cap)
{
    return n_cells < 0 || cap < 0 ? 0 : bsig::narrow_message_bytes(n_cells, cap);
}

int bsig_narrow_pack(bsig_ctx *ctx, const int32_t *src_dev, int64_t n_cells, void *msg_dev, int64_t cap)
{
    if (!ctx || !msg_dev || (n_cells > 0 && !src_dev) || n_cells < 0 || cap < 0) return fail(BSIG_ERR_ARG, "bad argument to bsig_narrow_pack");
    if (((uintptr_t)src_dev & 15) != 0 || ((uintptr_t)msg_dev & 15) != 0) return fail(BSIG_ERR_ARG, "device buffers must be 16-byte aligned");
    if (n_cells > (int64_t)UINT32_MAX) return fail(BSIG_ERR_ARG, "a narrow message holds at most 2^32 - 1 cells (an exception names its cell in 32 bits)");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(bsig::launch_narrow_pack(src_dev, n_cells, msg_dev, cap, ctx->stream));
    return BSIG_OK;
}

int bsig_narrow_count(bsig_ctx *ctx, const void *msg_dev, int64_t *n_exceptions)
{
    if (!ctx || !msg_dev || !n_exceptions) return fail(BSIG_ERR_ARG, "NULL argument to bsig_narrow_count");
    HIP_TRY(hipSetDevice(ctx->device));
    uint32_t k = 0;
    HIP_TRY(hipMemcpyAsync(&k, msg_dev, sizeof k, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *n_exceptions = (int64_t)k;
    return BSIG_OK;
}

int bsig_segmap_run_narrow(bsig_segmap *M, const void *msg_dev, int64_t n_cells, int64_t cap, int32_t *dst_dev)
{
    if (!M) return fail(BSIG_ERR_ARG, "segment map is NULL");
    if (M->n == 0) return BSIG_OK;
    if (!msg_dev || !dst_dev || n_cells < 0 || cap < 0) return fail(BSIG_ERR_ARG, "bad argument to bsig_segmap_run_narrow");
    if (n_cells < M->src_cells) return fail(BSIG_ERR_ARG, "the message codes %lld cells, the map's segments span %lld", (long long)n_cells, (long long)M->src_cells);
    if (((uintptr_t)msg_dev & 15) != 0) return fail(BSIG_ERR_ARG, "device buffers must be 16-byte aligned");
    HIP_TRY(hipSetDevice(M->ctx->device));
    HIP_TRY(bsig::launch_place_narrow(M->n, msg_dev, n_cells, cap, M->d_src_off, dst_dev, M->d_dst_off, M->d_which, M->d_overflow, M->ctx->stream));
    return BSIG_OK;
}

int bsig_segmap_narrow_overflowed(bsig_segmap *M, int *overflowed)
{
    if (!M || !overflowed) return fail(BSIG_ERR_ARG, "NULL argument to bsig_segmap_narrow_overflowed");
    HIP_TRY(hipSetDevice(M->ctx->device));
    HIP_TRY(hipMemcpyAsync(overflowed, M->d_overflow, sizeof(int), hipMemcpyDeviceToHost, M->ctx->stream));
    HIP_TRY(hipStreamSynchronize(M->ctx->stream));
    return BSIG_OK;
}

void bsig_segmap_free(bsig_segmap *M)
{
    if (!M) return;
    (void)hipSetDevice(M->ctx->device);
    if (M->d_overflow) (void)hipFree(M->d_overflow);
    if (M->d_src_off) (void)hipFree(M->d_src_off);
    if (M->d_dst_off) (void)hipFree(M->d_dst_off);
    if (M->d_which) (void)hipFree(M->d_which);
    delete M;
}

// FNV-1a over the BGZF block table as the device-side decode builds it
static uint64_t block_table_checksum(const bsig::BgzfFile &f)
{
    uint64_t h = 1469598103934665603ull;
    for (const bsig::BgzfBlock &b : f.blocks())
        for (uint64_t v : {(uint64_t)b.coff, (uint64_t)b.csize, (uint64_t)b.doff, (uint64_t)b.dlen, (uint64_t)b.isize, (uint64_t)b.crc}) {
            h ^= v;
            h *= 1099511628211ull;
        }
    return h;
}

int bsig_debug_block_table(const char *path, int64_t *n_blocks, uint64_t *checksum)
{
    // (env BAMSIGNALS_SCAN=mmap|pread picks the walk: tests compare the two walks)
    if (!path || !n_blocks || !checksum) return fail(BSIG_ERR_ARG, "NULL argument");
    bsig::BgzfFile f;
    const int rc = f.open(path);
    if (rc) return rc;
    *n_blocks = (int64_t)f.blocks().size();
    *checksum = block_table_checksum(f);
    return BSIG_OK;
}

int bsig_debug_block_table_progressive(const char *path, int64_t head_bytes, int64_t *n_head, int64_t *n_blocks, uint64_t *checksum)
{
    // the same table in two steps (BgzfFile::open_progressive): *n_head = blocks tabulated before the rest was
    // waited for (== *n_blocks when the file was tabulated whole at once)
    if (!path || !n_head || !n_blocks || !checksum || head_bytes <= 0) return fail(BSIG_ERR_ARG, "bad argument");
    bsig::BgzfFile f;
    int rc = f.open_progressive(path, (uint64_t)head_bytes);
    if (rc) return rc;
    *n_head = (int64_t)f.blocks().size();
    rc = f.finish();
    if (rc) return rc;
    *n_blocks = (int64_t)f.blocks().size();
    *checksum = block_table_checksum(f);
    return BSIG_OK;
}

}  // extern "C"
