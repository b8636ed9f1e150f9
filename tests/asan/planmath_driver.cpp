// Test-only driver for the arithmetic of plan creation (bamsignals_amd/csrc/planmath.h), built with
// -fsanitize=address,undefined (make -C bamsignals_amd/csrc planmath; tests/test_planmath_cpu.py).  It includes that
// header and nothing else of the library.  Commands come as whitespace-separated integers on standard input, every answer
// is one or more lines of integers:
//   rule     := mode cov_ex binsize ss mid tspan frag_len ext lay_binsize overlap minoverlap
//   kind     := sum xcorr xcorr_body max_lag frag len_bin own_tile_cells row_tiles
//   tilesize rule kind caller_tile_cells n len[n]              ->  cells xbody
//   kparams  rule kind caller_tile_cells tile_cells quad_off  mapqual requiredF filteredF n_tlen_filter tf0 tf1 shift
//            (n maxspan kshift has_p5h p5h_off)[5]  n_codes codes[n_codes]
//                                                              ->  rel24 packed_half short_half short_off[2] short_win[2]
//                                                                  div_magic div_shift div_m15 div_s15 use_tlen shift overlap_wide
//   div15                                                      ->  "ok" after checking every binsize 2..8192 (see below)
//   tiles    rule kind caller_tile_cells n_ref (unit0 units)[n_ref] n (rid loc len strand)[n] off[n + 1]
//                                                              ->  cells xbody kernel_mode needs_zero n_items, then per tile
//                                                                  loc len c0 nc out_off ref_unit0 units_strand
//   heavy    heavy_reads slice_reads policy count_mode coverage n (nc (x y)[5])[n]
//                                                              ->  reads of every tile; the depth bound of all tiles;
//                                                                  n_heavy_tiles heavy_sq n_hitems; the main tiles' flags;
//                                                                  per heavy item: its tile, its flags, (x y)[5] (slices only)
//   runs     per ceiling n_wide n weight[n]                    ->  the runs as a b pairs
//   sumruns  per S n (c0 nc)[n] m (c0 nc)[m]                   ->  main runs; all runs as a b pairs; the chunks as slot_lo
//                                                                  slot_hi cell0 nvals; max_nvals
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../bamsignals_amd/csrc/planmath.h"

static long long get()
{
    long long v = 0;
    if (scanf("%lld", &v) != 1) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}

static bsig::PlanRule get_rule()
{
    bsig::PlanRule r{};
    r.mode = (int)get(); r.cov_ex = get() != 0; r.binsize = (int32_t)get(); r.ss = get() != 0; r.mid = get() != 0; r.tspan = get() != 0;
    r.frag_len = (int32_t)get(); r.ext = get(); r.lay_binsize = (int32_t)get(); r.overlap = (int)get(); r.minoverlap = (int32_t)get();
    r.threads = 256;
    return r;
}

static bsig::KindFacts get_kind()
{
    bsig::KindFacts k;
    k.sum = get() != 0; k.xcorr = get() != 0; k.xcorr_body = (int32_t)get(); k.max_lag = (int32_t)get(); k.frag = get() != 0;
    k.len_bin = (int32_t)get(); k.own_tile_cells = (int32_t)get(); k.row_tiles = get() != 0;
    return k;
}

// div15 for every binsize 2..8192, at every multiple of the binsize below 2^15 and the value before it: the quotient is
// exact and the product fits 32 bits; no multiplier outside 2..8192
static bool div15_holds()
{
    uint32_t m; int32_t s;
    for (int32_t b : {-1, 0, 1, 8193, 65536}) {
        bsig::div15(b, &m, &s);
        if (m != 0 || s != 0) return false;
    }
    for (int32_t b = 2; b <= 8192; ++b) {
        bsig::div15(b, &m, &s);
        if (m == 0 || m >= (1u << 17)) return false;
        for (uint64_t k = b; k <= (1u << 15); k += b)
            for (uint64_t n : {k - 1, k}) {
                if (n >= (1u << 15)) continue;
                if (n * m >= ((uint64_t)1 << 32) || (n * m) >> s != n / b) return false;
            }
    }
    return true;
}

int main()
{
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        if (!strcmp(cmd, "tilesize")) {
            const bsig::PlanRule r = get_rule();
            const bsig::KindFacts kf = get_kind();
            const int caller = (int)get();
            std::vector<int32_t> len((size_t)get());
            for (auto &v : len) v = (int32_t)get();
            const bsig::TileSize ts = bsig::tile_cells_for(r, caller, (int64_t)len.size(), len.data(), kf);
            printf("%d %d\n", ts.cells, ts.xbody);
        } else if (!strcmp(cmd, "kparams")) {
            const bsig::PlanRule r = get_rule();
            const bsig::KindFacts kf = get_kind();
            bsig_params prm{};
            prm.tile_cells = (int32_t)get();
            const int tile = (int)get();
            const bool quad_off = get() != 0;
            prm.mapqual = (int32_t)get(); prm.requiredF = (int32_t)get(); prm.filteredF = (int32_t)get();
            prm.n_tlen_filter = (int32_t)get(); prm.tlen_filter[0] = (int32_t)get(); prm.tlen_filter[1] = (int32_t)get();
            prm.shift = (int32_t)get();
            bsig::LayoutFacts L{};
            for (auto &C : L.cls) {
                C.n = get(); C.maxspan = (int32_t)get(); C.kshift = (int32_t)get(); C.has_p5h = get() != 0; C.p5h_off = (uint32_t)get();
            }
            std::vector<uint32_t> codes((size_t)get());
            for (auto &c : codes) c = (uint32_t)get();
            L.codes = codes.data(); L.n_codes = (int32_t)codes.size();
            BsigKParams K{};
            bsig::fill_kparams(K, prm, r, tile, L, kf, quad_off);
            printf("%d %d %d %u %u %d %d %u %d %u %d %d %d %d\n", K.rel24, K.packed_half, K.short_half, K.short_off[0], K.short_off[1],
                   K.short_win[0], K.short_win[1], K.div_magic, K.div_shift, K.div_m15, K.div_s15, K.use_tlen, K.shift, K.overlap_wide);
        } else if (!strcmp(cmd, "div15")) {
            printf("%s\n", div15_holds() ? "1" : "0");
        } else if (!strcmp(cmd, "tiles")) {
            const bsig::PlanRule r = get_rule();
            const bsig::KindFacts kf = get_kind();
            const int caller = (int)get();
            const size_t n_ref = (size_t)get();
            std::vector<uint32_t> unit0(n_ref), units(n_ref);
            for (size_t k = 0; k < n_ref; ++k) { unit0[k] = (uint32_t)get(); units[k] = (uint32_t)get(); }
            const size_t n = (size_t)get();
            std::vector<int32_t> rid(n), loc(n), len(n), strand(n);
            for (size_t i = 0; i < n; ++i) { rid[i] = (int32_t)get(); loc[i] = (int32_t)get(); len[i] = (int32_t)get(); strand[i] = (int32_t)get(); }
            std::vector<int64_t> off(n + 1), order;
            for (auto &v : off) v = get();
            bsig::sort_ranges((int64_t)n, rid.data(), loc.data(), order);
            const bsig::TileSize ts = bsig::tile_cells_for(r, caller, (int64_t)n, len.data(), kf);
            const bsig::Tiles T = bsig::cut_tiles(order, rid.data(), loc.data(), len.data(), strand.data(), off.data(), unit0.data(),
                                                  units.data(), r, caller, ts, kf);
            printf("%d %d %d %d %zu\n", ts.cells, ts.xbody, T.kernel_mode, (int)T.needs_zero, T.items.size());
            for (const BsigWorkItem &w : T.items)
                printf("%d %d %d %d %lld %u %u\n", w.loc, w.len, w.c0, w.nc, (long long)w.out_off, w.ref_unit0, w.units_strand);
        } else if (!strcmp(cmd, "heavy")) {
            const int64_t heavy_reads = get(), slice_reads = get();
            const bsig::HeavyPolicy policy = get() ? bsig::kWalkWhole : bsig::kSlice;
            const bool count_mode = get() != 0, coverage = get() != 0;
            const size_t n = (size_t)get();
            std::vector<BsigWorkItem> items(n);
            std::vector<bsig::Pair32> win(n * BSIG_MAX_CLASSES);
            for (size_t t = 0; t < n; ++t) {
                items[t] = BsigWorkItem{};
                items[t].c0 = (int32_t)t;                // (a slice is told from its tile's by this)
                items[t].nc = (int32_t)get();
                for (int c = 0; c < BSIG_MAX_CLASSES; ++c) { win[t * BSIG_MAX_CLASSES + c].x = (uint32_t)get(); win[t * BSIG_MAX_CLASSES + c].y = (uint32_t)get(); }
            }
            const std::vector<int64_t> reads = bsig::reads_of_tiles(win);
            for (int64_t v : reads) printf("%lld ", (long long)v);
            printf("\n%.0Lf\n", bsig::depth_bound(items, reads, 0, n, coverage));
            const bsig::HeavySplit H = bsig::split_heavy(items, win, reads, heavy_reads, slice_reads, policy, count_mode);
            printf("%lld %.0Lf %zu\n", (long long)H.n_heavy_tiles, H.heavy_sq, H.hitems.size());
            for (const BsigWorkItem &w : items) printf("%u ", w.units_strand);
            printf("\n");
            if (H.hwin.size() != (policy == bsig::kSlice ? H.hitems.size() * BSIG_MAX_CLASSES : 0)) return 3;
            for (size_t k = 0; k < H.hitems.size(); ++k) {
                printf("%d %u", H.hitems[k].c0, H.hitems[k].units_strand);
                for (int c = 0; c < BSIG_MAX_CLASSES && policy == bsig::kSlice; ++c)
                    printf(" %u %u", H.hwin[k * BSIG_MAX_CLASSES + c].x, H.hwin[k * BSIG_MAX_CLASSES + c].y);
                printf("\n");
            }
        } else if (!strcmp(cmd, "runs")) {
            const int64_t per = get(), ceiling = get(), n_wide = get();
            std::vector<int64_t> weight((size_t)get());
            for (auto &v : weight) v = get();
            std::vector<bsig::Pair32> runs;
            bsig::cut_runs((int64_t)weight.size(), per, ceiling, [&](int64_t t) { return weight[(size_t)t]; }, runs);
            bsig::append_wide_runs(n_wide, runs);
            for (const bsig::Pair32 &q : runs) printf("%u %u ", q.x, q.y);
            printf("\n");
        } else if (!strcmp(cmd, "sumruns")) {
            const int64_t per = get();
            const int32_t S = (int32_t)get();
            std::vector<bsig::Pair32> runs;
            std::vector<BsigSumChunk> chunks;
            int32_t max_nvals = 0;
            for (int part = 0; part < 2; ++part) {
                std::vector<BsigWorkItem> it((size_t)get());
                for (auto &w : it) { w = BsigWorkItem{}; w.c0 = (int32_t)get(); w.nc = (int32_t)get(); }
                max_nvals = std::max(max_nvals, bsig::cut_sum_runs(it, per, S, runs, chunks));
                if (part == 0) printf("%zu\n", runs.size());
            }
            for (const bsig::Pair32 &q : runs) printf("%u %u ", q.x, q.y);
            printf("\n");
            for (const BsigSumChunk &c : chunks) printf("%u %u %d %d ", c.slot_lo, c.slot_hi, c.cell0, c.nvals);
            printf("\n%d\n", max_nvals);
        } else {
            return 2;
        }
    }
    return 0;
}
