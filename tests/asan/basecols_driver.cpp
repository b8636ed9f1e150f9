// Test-only driver for the host maker of the base columns (bamsignals_amd/csrc/bamio.cpp: bam_decode_bases), built with
// -fsanitize=address,undefined (make -C bamsignals_amd/csrc basecols; tests/test_nucleotides_asan_cpu.py).  Every file named
// on the command line is decoded whole and, where <file>.bai loads, through the index; what comes back is checked against
// itself and read through to its last byte (the nucleotide walk of nucmath.h's rules over every read), so that a column that
// promises more than it holds is found here.  A malformed input must end in a clean error; anything the sanitizers find
// aborts the process.  One line per file: "ok <reads> <bases> <checksum> <the regions' checksum>" or "err <code>: <message>" --
// a whole-file decode whose index-driven decode fails (the index of a damaged copy points anywhere) is "ok ... regions-err" --;
// the exit code is 0.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../bamsignals_amd/csrc/bamio.h"
#include "../../bamsignals_amd/csrc/host_util.h"
#include "../../bamsignals_amd/csrc/nucmath.h"

namespace bsig {
thread_local std::string g_last_error;
int fail(int code, const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}
}  // namespace bsig

// the columns against themselves, and a checksum of every count the walk would make on an endless reference
static bool walk(const bsig::HostColumns &c, const bsig::HostBases &b, uint64_t *sum)
{
    const int64_t n = c.size();
    if ((int64_t)b.seq_off.size() != n + 1 || (int64_t)c.cigar_off.size() != n + 1 || b.seq_off[0] != 0) return false;
    if ((int64_t)b.qual.size() != b.n_bases() || (int64_t)b.seq.size() != (b.n_bases() + 1) / 2) return false;
    if ((int64_t)c.cigar.size() != c.cigar_off[(size_t)n]) return false;
    uint64_t h = 1469598103934665603ull;
    for (int64_t k = 0; k < n; ++k) {
        const int64_t s0 = b.seq_off[(size_t)k], l_seq = b.seq_off[(size_t)k + 1] - s0;
        if (l_seq < 0 || c.cigar_off[(size_t)k] > c.cigar_off[(size_t)k + 1]) return false;
        const uint32_t *ops = c.cigar.data() + c.cigar_off[(size_t)k];
        const int64_t n_ops = c.cigar_off[(size_t)k + 1] - c.cigar_off[(size_t)k];
        h = (h ^ (uint64_t)bsig::nuc_clamped_end(c.pos[(size_t)k], bsig::nuc_ref_span(n_ops, [&](int64_t q) { return ops[q]; }))) * 1099511628211ull;
        int64_t q = 0;
        for (int64_t o = 0; o < n_ops; ++o) {
            const uint32_t op = ops[o] & 15u;
            const int64_t len = ops[o] >> 4;
            if (bsig::nuc_op_aligns(op))
                for (int64_t i = q; i < q + len && i < l_seq; ++i) {
                    const int64_t g = s0 + i;
                    const uint32_t byte = b.seq[(size_t)(g >> 1)];
                    h = (h ^ (bsig::nuc_channel((g & 1) ? byte & 15u : byte >> 4) << 8 | b.qual[(size_t)g])) * 1099511628211ull;
                }
            if (bsig::nuc_op_moves_query(op)) q += len;
        }
    }
    *sum = h;
    return true;
}

static void one(const std::string &path)
{
    bsig::BamHeader hdr;
    bsig::HostColumns cols;
    bsig::HostBases bases;
    uint64_t sum = 0, sum_r = 0;
    int rc = bsig::bam_decode_bases(path, nullptr, {}, 3, hdr, cols, bases);
    if (rc) { printf("err %d: %s\n", rc, bsig::g_last_error.c_str()); return; }
    if (!walk(cols, bases, &sum)) { printf("columns do not fit each other\n"); exit(4); }
    const int64_t n = cols.size(), n_bases = bases.n_bases();
    bsig::BaiIndex idx;
    if (bsig::bai_load(path + ".bai", idx) == 0 && !hdr.lens.empty()) {
        std::vector<bsig::Region> rg;
        for (size_t r = 0; r < hdr.lens.size() && r < idx.refs.size(); ++r) {
            rg.push_back(bsig::Region{(int32_t)r, 0, hdr.lens[r] / 2});
            rg.push_back(bsig::Region{(int32_t)r, hdr.lens[r] / 2, (int64_t)hdr.lens[r] + 1});
        }
        bsig::BamHeader h2;
        rc = bsig::bam_decode_bases(path, &idx, rg, 3, h2, cols, bases);
        if (rc) { printf("ok %lld %lld %016llx regions-err %d: %s\n", (long long)n, (long long)n_bases, (unsigned long long)sum, rc, bsig::g_last_error.c_str()); return; }
        if (!walk(cols, bases, &sum_r)) { printf("columns of the regions do not fit each other\n"); exit(4); }
    }
    printf("ok %lld %lld %016llx %016llx\n", (long long)n, (long long)n_bases, (unsigned long long)sum, (unsigned long long)sum_r);
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: basecols_driver <bam> [<bam> ...]\n"); return 2; }
    for (int k = 1; k < argc; ++k) one(argv[k]);
    return 0;
}
