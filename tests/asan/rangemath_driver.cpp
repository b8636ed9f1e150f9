// Test-only driver for the range arithmetic of the file-level calls (bamsignals_amd/csrc/rangemath.h), built with
// -fsanitize=address,undefined (make -C bamsignals_amd/csrc rangemath; tests/test_rangemath_cpu.py).  It includes that
// header and nothing else of the library.  Commands come as whitespace-separated integers on standard input, every answer
// is a line of integers:
//   deal n nd block  order[n]             (block 0: the default)  ->  the block, then per slot "w" + its ranges and
//                                                                      "r" + its runs as j0 j1 pairs
//   cut nd budget n  cells[n]                                     ->  per block: slot a b cells
//   cover m  (rid beg end)[m]  q  (rid beg end)[q]                ->  the merged intervals; covered? per query, then for all
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../bamsignals_amd/csrc/rangemath.h"

static bool next(long long *v) { return scanf("%lld", v) == 1; }

static void read_triples(long long m, std::vector<int32_t> &rid, std::vector<int64_t> &beg, std::vector<int64_t> &end)
{
    for (long long i = 0, r, b, e; i < m && next(&r) && next(&b) && next(&e); ++i) {
        rid.push_back((int32_t)r); beg.push_back(b); end.push_back(e);
    }
}

int main()
{
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        if (!strcmp(cmd, "deal")) {
            long long n, nd, block;
            if (!next(&n) || !next(&nd) || !next(&block)) return 2;
            std::vector<int64_t> order((size_t)n);
            for (auto &o : order) { long long v; if (!next(&v)) return 2; o = v; }
            if (!block) block = bsig::default_shard_block(n, (size_t)nd);
            const bsig::ShardDeal D = bsig::deal_shards(n, order, (size_t)nd, block);
            printf("%lld %lld\n", block, (long long)D.n_runs);
            for (size_t k = 0; k < (size_t)nd; ++k) {
                printf("w");
                for (int64_t i : D.which[k]) printf(" %lld", (long long)i);
                printf("\nr");
                for (const bsig::SegRun &q : D.runs[k]) printf(" %lld %lld", (long long)q.j0, (long long)q.j1);
                printf("\n");
            }
        } else if (!strcmp(cmd, "cut")) {
            long long nd, budget, n;
            if (!next(&nd) || !next(&budget) || !next(&n)) return 2;
            std::vector<int64_t> cells((size_t)n);
            for (auto &c : cells) { long long v; if (!next(&v)) return 2; c = v; }
            const std::vector<bsig::CellBlock> blocks = bsig::cut_blocks(cells, (size_t)nd, budget);
            printf("%zu\n", blocks.size());
            for (const bsig::CellBlock &B : blocks) printf("%zu %lld %lld %lld\n", B.slot, (long long)B.a, (long long)B.b, (long long)B.cells);
            for (size_t k = 0; k < (size_t)nd; ++k) {
                int64_t a, b;
                bsig::slot_block(n, k, (size_t)nd, &a, &b);
                printf("%lld %lld\n", (long long)a, (long long)b);
            }
        } else if (!strcmp(cmd, "cover")) {
            long long m, q;
            std::vector<int32_t> rid, qrid;
            std::vector<int64_t> beg, end, qbeg, qend;
            if (!next(&m)) return 2;
            read_triples(m, rid, beg, end);
            if (!next(&q)) return 2;
            read_triples(q, qrid, qbeg, qend);
            bsig::Intervals R;
            bsig::set_coverage(R, m, rid.data(), beg.data(), end.data());
            printf("%zu", R.rid.size());
            for (size_t i = 0; i < R.rid.size(); ++i) printf(" %d %lld %lld", R.rid[i], (long long)R.beg[i], (long long)R.end[i]);
            printf("\n");
            for (long long i = 0; i < q; ++i) printf("%d ", (int)bsig::regions_covered(R, 1, &qrid[(size_t)i], &qbeg[(size_t)i], &qend[(size_t)i]));
            printf("%d\n", (int)bsig::regions_covered(R, q, qrid.data(), qbeg.data(), qend.data()));
        } else {
            return 2;
        }
    }
    return 0;
}
