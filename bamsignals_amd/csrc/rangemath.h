// The range arithmetic of the file-level calls: how sorted ranges are dealt to GPU slots, cut into blocks, and which
// regions an index-driven decode covers.  Plain integers and vectors only -- no HIP, no ABI types -- so that a host program
// can call it (tests/asan/rangemath_driver.cpp does, under the sanitizers).
#ifndef BSIG_RANGEMATH_H
#define BSIG_RANGEMATH_H
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace bsig {

// How the (rid, loc)-sorted ranges are shared out to nd GPU slots in contiguous shares: slot k takes order[a .. b), empty
// where there are fewer ranges than slots.
inline void slot_block(int64_t n, size_t k, size_t nd, int64_t *a, int64_t *b)
{
    *a = n * (int64_t)k / (int64_t)nd;
    *b = n * (int64_t)(k + 1) / (int64_t)nd;
}

// The per-range result's dealer: the sorted ranges go out in BLOCKS of consecutive ranges (block b to slot b mod nd; by
// default at least eight blocks per slot, at most 4,096 ranges per block): still balanced over the genome, and where the
// caller's order is the sorted order -- tilings, sorted peaks -- a block is one contiguous slice of the caller's result.
inline int64_t default_shard_block(int64_t n, size_t nd)
{
    return std::max<int64_t>(1, std::min<int64_t>(n / (int64_t)(nd * 8), 4096));
}
struct SegRun { int64_t j0, j1; };                 // segments [j0, j1) of a shard
struct ShardDeal {
    std::vector<std::vector<int64_t>> which;       // per slot: the caller's indices of its ranges, in sorted order
    std::vector<std::vector<SegRun>> runs;         // ... and its maximal runs of indices consecutive in the caller's order:
    int64_t n_runs = 0;                            //     contiguous slices of the caller's result
};
inline ShardDeal deal_shards(int64_t n, const std::vector<int64_t> &order, size_t nd, int64_t block)
{
    ShardDeal D;
    D.which.resize(nd);
    D.runs.resize(nd);
    for (auto &w : D.which) w.reserve((size_t)n / nd + 1);
    for (int64_t k = 0; k < n; ++k) D.which[(size_t)((k / block) % (int64_t)nd)].push_back(order[(size_t)k]);
    for (size_t k = 0; k < nd; ++k) {
        const std::vector<int64_t> &w = D.which[k];
        for (size_t j = 0; j < w.size();) {
            size_t e = j + 1;
            while (e < w.size() && w[e] == w[e - 1] + 1) ++e;
            D.runs[k].push_back(SegRun{(int64_t)j, (int64_t)e});
            j = e;
        }
        D.n_runs += (int64_t)D.runs[k].size();
    }
    return D;
}

// The encoded results' cutter: every slot's share (slot_block) of the sorted ranges in blocks of at most `budget` cells; a
// single larger range is a block of its own.  cells[i]: the cells of sorted range i.
struct CellBlock {
    int64_t a = 0, b = 0, cells = 0;               // sorted ranges [a, b)
    size_t slot = 0;
};
inline std::vector<CellBlock> cut_blocks(const std::vector<int64_t> &cells, size_t nd, int64_t budget)
{
    std::vector<CellBlock> blocks;
    for (size_t k = 0; k < nd; ++k) {
        int64_t a, b;
        slot_block((int64_t)cells.size(), k, nd, &a, &b);
        for (int64_t i = a; i < b;) {
            CellBlock B;
            B.a = i; B.slot = k;
            B.cells = cells[(size_t)i++];
            while (i < b && B.cells + cells[(size_t)i] <= budget) B.cells += cells[(size_t)i++];
            B.b = i;
            blocks.push_back(B);
        }
    }
    return blocks;
}

// The intervals an index-driven decode was made for: merged, sorted by reference and start.
struct Intervals {
    std::vector<int32_t> rid;
    std::vector<int64_t> beg, end;
};
inline void set_coverage(Intervals &R, int64_t n, const int32_t *rid, const int64_t *beg, const int64_t *end)
{
    std::vector<int64_t> order((size_t)n);
    for (int64_t i = 0; i < n; ++i) order[(size_t)i] = i;
    std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return rid[a] != rid[b] ? rid[a] < rid[b] : beg[a] < beg[b]; });
    R.rid.clear(); R.beg.clear(); R.end.clear();
    for (int64_t k = 0; k < n; ++k) {
        const int64_t i = order[(size_t)k];
        if (end[i] <= beg[i]) continue;
        if (!R.rid.empty() && R.rid.back() == rid[i] && beg[i] <= R.end.back()) {
            R.end.back() = std::max(R.end.back(), end[i]);
        } else {
            R.rid.push_back(rid[i]); R.beg.push_back(beg[i]); R.end.push_back(end[i]);
        }
    }
}
// ... which serve a later query whose every region lies inside one of them: the index query of the earlier call returned
// every record overlapping its intervals, hence every record overlapping a sub-interval
inline bool regions_covered(const Intervals &R, int64_t n, const int32_t *rid, const int64_t *beg, const int64_t *end)
{
    const size_t m = R.rid.size();
    for (int64_t i = 0; i < n; ++i) {
        if (end[i] <= beg[i]) continue;
        // last interval with (rid, beg) <= (rid[i], beg[i])
        size_t lo = 0, hi = m;
        while (lo < hi) {
            const size_t mid = (lo + hi) / 2;
            if (R.rid[mid] < rid[i] || (R.rid[mid] == rid[i] && R.beg[mid] <= beg[i])) lo = mid + 1; else hi = mid;
        }
        if (lo == 0) return false;
        const size_t k = lo - 1;
        if (R.rid[k] != rid[i] || R.end[k] < end[i]) return false;
    }
    return true;
}

}  // namespace bsig
#endif
