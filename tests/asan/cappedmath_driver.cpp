// Test-only driver for the capped plans' arithmetic (bamsignals_amd/csrc/planmath.h: capped_binsize, capped_tile_bins,
// capped_widen, capped_window, and the tile cutter with KindFacts::capped), built with -fsanitize=address,undefined
// (make -C bamsignals_amd/csrc cappedmath; tests/test_capped_cpu.py).  It includes that header and nothing else of the
// library.  Commands come as whitespace-separated integers on standard input, every answer is one line of integers:
//   binsize  lay_binsize                       ->  the bins' width the kernel divides by
//   tilebins tile_cells binsize                ->  the accumulators a row, then the most bins any tile of tile_cells cells
//                                                  touches, counted over every c0 in 0 .. 3 * binsize (brute force; 0 where
//                                                  there are no accumulators)
//   widen    loc len frag_len                  ->  fits loc len lead
//   window   u lead frag_len                   ->  f_hi f_lo r_hi r_lo
//   tiles    tile_cells n (loc len strand off)[n] off[n]
//                                              ->  n_items, then per tile on its own line: loc len c0 nc out_off neg
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

int main()
{
    char cmd[32];
    while (scanf("%31s", cmd) == 1) {
        if (!strcmp(cmd, "binsize")) {
            printf("%d\n", (int)bsig::capped_binsize((int32_t)get()));
        } else if (!strcmp(cmd, "tilebins")) {
            const int32_t tile_cells = (int32_t)get(), binsize = (int32_t)get();
            const int32_t n_acc = bsig::capped_tile_bins(tile_cells, binsize);
            long long most = 0;
            for (long long c0 = 0; n_acc > 0 && c0 <= 3ll * binsize && c0 < (1ll << 22); ++c0)
                most = std::max(most, (c0 + tile_cells - 1) / binsize - c0 / binsize + 1);
            printf("%d %lld\n", (int)n_acc, most);
        } else if (!strcmp(cmd, "widen")) {
            const int32_t loc = (int32_t)get(), len = (int32_t)get(), frag_len = (int32_t)get();
            const bsig::CappedWide c = bsig::capped_widen(loc, len, frag_len);
            printf("%d %d %d %d\n", c.fits ? 1 : 0, (int)c.loc, (int)c.len, (int)c.lead);
        } else if (!strcmp(cmd, "window")) {
            const int32_t u = (int32_t)get(), lead = (int32_t)get(), frag_len = (int32_t)get();
            const bsig::CappedIdx w = bsig::capped_window(u, lead, frag_len);
            printf("%lld %lld %lld %lld\n", (long long)w.f_hi, (long long)w.f_lo, (long long)w.r_hi, (long long)w.r_lo);
        } else if (!strcmp(cmd, "tiles")) {
            const int tile_cells = (int)get();
            const long long n = get();
            std::vector<int32_t> rid((size_t)n, 0), loc((size_t)n), len((size_t)n), strand((size_t)n);
            std::vector<int64_t> off((size_t)n + 1), order((size_t)n);
            for (long long i = 0; i < n; ++i) {
                loc[(size_t)i] = (int32_t)get(); len[(size_t)i] = (int32_t)get(); strand[(size_t)i] = (int32_t)get();
                off[(size_t)i] = get();
                order[(size_t)i] = i;
            }
            off[(size_t)n] = get();
            const uint32_t unit0 = 0, units = 100;
            bsig::PlanRule r{};
            r.mode = BSIG_MODE_PROFILE; r.binsize = 1; r.ss = true; r.lay_binsize = 1; r.threads = 256;
            bsig::KindFacts kf;
            kf.own_tile_cells = tile_cells; kf.capped = true;
            const bsig::TileSize ts = bsig::tile_cells_for(r, 0, n, len.data(), kf);
            const bsig::Tiles T = bsig::cut_tiles(order, rid.data(), loc.data(), len.data(), strand.data(), off.data(), &unit0, &units, r,
                                                  0, ts, kf);
            printf("%zu\n", T.items.size());
            for (const BsigWorkItem &w : T.items)
                printf("%d %d %d %d %lld %d\n", (int)w.loc, (int)w.len, (int)w.c0, (int)w.nc, (long long)w.out_off,
                       (w.units_strand & BSIG_ITEM_NEG) ? 1 : 0);
        } else {
            fprintf(stderr, "unknown command %s\n", cmd);
            return 2;
        }
    }
    return 0;
}
