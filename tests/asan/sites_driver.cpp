// Stand-alone driver of the site decision (csrc/sitemath.h: the parameter rule and site_classify -- the function k_site_tiles
// runs on the device) for a CPU build with -fsanitize=address,undefined; tests/test_sites_asan_cpu.py writes its input and
// compares what it prints with tests/sites_expected.py.  Host code only: nothing of the library, no GPU.
//
// usage: sites_driver FILE...
// FILE, little endian: int32 min_depth, min_alt, frac_num, frac_den, alt_mask, planes (1 or 2), has_ref (0 or 1), n_ranges;
// n_ranges int32 widths; every range's cells int32 [plane][channel][position]; with has_ref every range's reference codes, a byte
// a cell.  Per file: "rule ok" or "rule <sentence>" (and nothing more), then a line per site "range pos alleles counts...", then
// "end <number of sites>".
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../bamsignals_amd/csrc/sitemath.h"

namespace {

bool read_all(FILE *f, void *dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, f) == bytes; }

int run(const char *path)
{
    FILE *f = fopen(path, "rb");
    if (!f) { printf("err cannot open %s\n", path); return 1; }
    int32_t head[8];
    if (!read_all(f, head, sizeof head)) { printf("err short header\n"); fclose(f); return 1; }
    const char *why = bsig::site_rule_sentence(head[0], head[1], head[2], head[3], head[4]);
    if (why) { printf("rule %s\n", why); fclose(f); return 0; }
    printf("rule ok\n");
    const bsig::SiteParams prm{head[0], head[1], head[2], head[3], (uint32_t)head[4]};
    const int planes = head[5];
    const bool has_ref = head[6] != 0;
    const int32_t n = head[7];
    if ((planes != 1 && planes != 2) || n < 0) { printf("err bad header\n"); fclose(f); return 1; }
    std::vector<int32_t> width((size_t)n);
    if (!read_all(f, width.data(), (size_t)n * sizeof(int32_t))) { printf("err short widths\n"); fclose(f); return 1; }
    std::vector<std::vector<int32_t>> cells((size_t)n);
    std::vector<std::vector<uint8_t>> ref((size_t)n);
    for (int32_t i = 0; i < n; ++i) {
        if (width[(size_t)i] < 0) { printf("err negative width\n"); fclose(f); return 1; }
        cells[(size_t)i].resize((size_t)planes * bsig::kNucChannels * (size_t)width[(size_t)i]);           // (its exact size: a read past it is reported)
        if (!read_all(f, cells[(size_t)i].data(), cells[(size_t)i].size() * sizeof(int32_t))) { printf("err short cells\n"); fclose(f); return 1; }
    }
    for (int32_t i = 0; has_ref && i < n; ++i) {
        ref[(size_t)i].resize((size_t)width[(size_t)i]);
        if (!read_all(f, ref[(size_t)i].data(), ref[(size_t)i].size())) { printf("err short ref\n"); fclose(f); return 1; }
    }
    fclose(f);
    long long n_sites = 0;
    for (int32_t i = 0; i < n; ++i) {
        const int64_t w = width[(size_t)i];
        const std::vector<int32_t> &c = cells[(size_t)i];
        for (int64_t p = 0; p < w; ++p) {
            int64_t sum[bsig::kNucChannels];
            for (int ch = 0; ch < bsig::kNucChannels; ++ch) {
                sum[ch] = c[(size_t)(ch * w + p)];
                if (planes == 2) sum[ch] += c[(size_t)((bsig::kNucChannels + ch) * w + p)];
            }
            const int32_t code = has_ref ? (int32_t)ref[(size_t)i][(size_t)p] : -1;
            if (code > bsig::kSiteRefN) { printf("err ref code %d\n", (int)code); return 1; }
            const int32_t k = bsig::site_classify(sum, code, prm);
            if (k < 0) continue;
            printf("%d %lld %d", (int)i, (long long)p, (int)k);
            for (int pl = 0; pl < planes; ++pl)
                for (int ch = 0; ch < bsig::kNucChannels; ++ch) printf(" %d", (int)c[(size_t)((pl * bsig::kNucChannels + ch) * w + p)]);
            printf("\n");
            ++n_sites;
        }
    }
    printf("end %lld\n", n_sites);
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    int rc = 0;
    for (int k = 1; k < argc; ++k) rc |= run(argv[k]);
    return rc;
}
