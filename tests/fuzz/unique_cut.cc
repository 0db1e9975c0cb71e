// Host check of the unique-row route of csrc/tile_cut.h (plain C++, built with the host sanitizers by tests/test_unique_cut_host.py).
//     unique_cut cut TILE_BLOCKS WPS N_ROWS REPS  c0 c1 ...
//         N_ROWS common rows whose 64-row blocks hold REPS representatives (a comma list, one number per block, the last block
//         may be partial); windows as pairs of common-row edges, no rare sites.  One line: "tiles=K split=a,b,..." with a tile as
//         head+mid[u0-u1)+tail: its head rows, its whole blocks with their range of the stream, its tail rows; "bytes=N".
//     unique_cut random SEED LISTS
//         LISTS seeded random matrices (rows, representatives per block, rare sites) and window lists, each checked as below;
//         every 16th list is long enough for tiles above UNIQ_MID_MAX whole blocks at tile_blocks 4096.  "random ok lists=N"
//     unique_cut bound
//         the 32-bit lane sums of the fixed-WPS kernel with weights, for every number of whole blocks a tile of tile_blocks <=
//         4096 at wps 16 can hold.  "bound ok worst=N"
// Properties of cut_tiles(..., ubase) against a model computed here row by row:
//   1 tiles, singles, wins are those of the cut without ubase; there is one UniqRange per tile
//   2 a tile's range is {ubase[g0], ubase[g1]} of the whole blocks [g0, g1) the model finds inside its rows when there are 1 ..
//     UNIQ_MID_MAX of them and the blocks of the stream that range touches, with their weights, are fewer bytes than the whole
//     blocks; else empty.  Non-empty ranges are ascending and disjoint over the tiles
//   3 every common row of a covered segment is in exactly one of: a head, a tail, a whole block of a mid range (a tile without a
//     range: all its rows are head) — and in none where no window covers it; a head and a tail lie inside one block each
//   4 bytes_streamed is the model's: per tile the head's and the tail's block, the blocks of the stream its range touches with 64
//     weight bytes each (without a range: its blocks of rows), 8 bytes per entry and the aligned words of its singletons
//   5 with a range, no lane of a 256-thread workgroup (a wave takes every fourth block of head | mid | tail in one running index)
//     is handed more than ceil((mid + 1) / 4) blocks of the stream, and uniq_lane_sum_bound of that stays below 2^32
// Exit 0, else exit 1 with the breached property on stderr.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "tile_cut.h"

using namespace impop;

#define CHECK(cond, ...)                                                      \
    do {                                                                      \
        if (!(cond)) {                                                        \
            fprintf(stderr, "BREACH %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                                     \
            fprintf(stderr, "\n");                                            \
            return 1;                                                         \
        }                                                                     \
    } while (0)
typedef unsigned long long ull;

static uint64_t g_rng;
static uint64_t rnd(uint64_t below) {  // splitmix64
    uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (z ^ (z >> 31)) % below;
}

// the kernel's hand-out: blocks of head | mid | tail from one running index, wave w takes index w, w + 4, ...; the most blocks of
// the stream one wave gets
static uint64_t most_mid_blocks_per_wave(uint64_t head_blocks, uint64_t mid_blocks_touched) {
    uint64_t per[4] = {0, 0, 0, 0};
    for (uint64_t i = 0; i < mid_blocks_touched; ++i) ++per[(head_blocks + i) & 3];
    return std::max(std::max(per[0], per[1]), std::max(per[2], per[3]));
}

// reps[g]: the representatives of block g of the n_rows common rows -> ubase, one entry per block and one past the last
static std::vector<uint64_t> prefix_of(const std::vector<uint32_t> &reps) {
    std::vector<uint64_t> ubase(reps.size() + 1, 0);
    for (size_t g = 0; g < reps.size(); ++g) ubase[g + 1] = ubase[g] + reps[g];
    return ubase;
}

static int check_cut(const std::vector<LayoutWindow> &w, uint32_t tile_blocks, uint32_t wps, bool packed, uint64_t n_rows,
                     const std::vector<uint64_t> &ubase, TileCut &cut) {
    cut = TileCut();
    cut_tiles(w, tile_blocks, wps, packed, cut, ubase.data());
    TileCut plain;
    cut_tiles(w, tile_blocks, wps, packed, plain);
    const size_t nt = cut.tiles.size();
    // 1
    CHECK(nt == plain.tiles.size() && cut.uniqs.size() == nt && plain.uniqs.empty() && cut.singles.size() == plain.singles.size(),
          "%zu tiles, %zu ranges; without the prefix %zu tiles", nt, cut.uniqs.size(), plain.tiles.size());
    for (size_t k = 0; k < nt; ++k) {
        const ScanTile &a = cut.tiles[k], &b = plain.tiles[k];
        CHECK(a.site_begin == b.site_begin && a.site_end == b.site_end && a.rare_begin == b.rare_begin && a.rare_end == b.rare_end,
              "tile %zu differs from the cut without the prefix", k);
        if (packed) CHECK(cut.singles[k].begin == plain.singles[k].begin && cut.singles[k].end == plain.singles[k].end, "tile %zu: singles differ", k);
    }
    for (size_t i = 0; i < w.size(); ++i)
        CHECK(cut.wins[i].t0 == plain.wins[i].t0 && cut.wins[i].t1 == plain.wins[i].t1 && cut.wins[i].n_sites == plain.wins[i].n_sites,
              "window %zu differs from the cut without the prefix", i);
    // the model: which rows some window holds; how often each is read, and as what
    std::vector<uint8_t> covered(n_rows + 1, 0), read(n_rows + 1, 0);
    for (const LayoutWindow &x : w)
        for (uint64_t s = x.lo.c; s < x.hi.c; ++s) covered[s] = 1;
    uint64_t bytes = 0, last_u = 0;
    for (size_t k = 0; k < nt; ++k) {
        const ScanTile &t = cut.tiles[k];
        const UniqRange u = cut.uniqs[k];
        // whole blocks inside the tile, block by block
        uint64_t g0 = 0, g1 = 0, whole = 0;
        if (t.site_end > t.site_begin)
            for (uint64_t g = t.site_begin / 64; g * 64 < t.site_end; ++g)
                if (g * 64 >= t.site_begin && (g + 1) * 64 <= t.site_end) {
                    if (!whole) g0 = g;
                    CHECK(!whole || g == g1, "tile %zu: whole blocks are not contiguous", k);
                    g1 = g + 1;
                    ++whole;
                }
        bool want = whole >= 1 && whole <= UNIQ_MID_MAX;
        if (want) {
            CHECK(g1 < ubase.size(), "tile %zu: block %llu has no prefix entry", k, (ull)g1);
            uint64_t touched = 0;
            for (uint64_t b = ubase[g0] / 64; b * 64 < ubase[g1]; ++b) ++touched;
            want = touched * (256ull * wps + 64) < whole * 256ull * wps;
        }
        // 2
        if (want) {
            CHECK(u.begin == ubase[g0] && u.end == ubase[g1] && u.end > u.begin, "tile %zu: range [%llu, %llu), blocks [%llu, %llu) hold [%llu, %llu)",
                  k, (ull)u.begin, (ull)u.end, (ull)g0, (ull)g1, (ull)ubase[g0], (ull)ubase[g1]);
            CHECK(u.begin >= last_u, "tile %zu: range starts at %llu before %llu", k, (ull)u.begin, (ull)last_u);
            last_u = u.end;
        } else {
            CHECK(u.begin == 0 && u.end == 0, "tile %zu: %llu whole blocks and a range [%llu, %llu)", k, (ull)whole, (ull)u.begin, (ull)u.end);
        }
        // 3: the split as the kernel makes it (mid_blocks) against the model's blocks
        const MidBlocks mb = mid_blocks(t.site_begin, t.site_end);
        const bool folded = u.end > u.begin;
        if (folded) CHECK(mb.any() && mb.g0 == g0 && mb.g1 == g1, "tile %zu: mid_blocks [%llu, %llu), model [%llu, %llu)", k, (ull)mb.g0, (ull)mb.g1, (ull)g0, (ull)g1);
        const uint64_t head_end = folded ? mb.g0 * 64 : t.site_end, tail_begin = folded ? mb.g1 * 64 : t.site_end;
        CHECK(t.site_begin <= head_end && head_end <= tail_begin && tail_begin <= t.site_end, "tile %zu: head / mid / tail out of order", k);
        for (uint64_t s = t.site_begin; s < head_end; ++s) ++read[s];
        for (uint64_t s = head_end; s < tail_begin; ++s) ++read[s];  // a row of a whole block: stands in its block's representatives
        for (uint64_t s = tail_begin; s < t.site_end; ++s) ++read[s];
        uint64_t rows = 0;
        if (folded) {
            const uint64_t head = head_end - t.site_begin, tail = t.site_end - tail_begin;
            CHECK(head < 64 && tail < 64, "tile %zu: head of %llu rows, tail of %llu", k, (ull)head, (ull)tail);
            if (head) CHECK(t.site_begin / 64 == (head_end - 1) / 64, "tile %zu: head spans blocks", k);
            if (tail) CHECK(tail_begin / 64 == (t.site_end - 1) / 64, "tile %zu: tail spans blocks", k);
            uint64_t ub = 0;  // blocks of the stream the range touches, counted one by one
            for (uint64_t b = u.begin / 64; b * 64 < u.end; ++b) ++ub;
            rows = ((head ? 1 : 0) + (tail ? 1 : 0) + ub) * 256ull * wps + ub * 64;
            // 5
            const uint64_t per_wave = most_mid_blocks_per_wave(head ? 1 : 0, ub);
            CHECK(ub <= whole + 1 && per_wave <= (whole + 1 + 3) / 4, "tile %zu: %llu blocks of the stream for %llu whole blocks, %llu for one wave", k,
                  (ull)ub, (ull)whole, (ull)per_wave);
            CHECK(uniq_lane_sum_bound(whole) < (1ull << 32), "tile %zu: %llu whole blocks: lane sums up to %llu", k, (ull)whole, (ull)uniq_lane_sum_bound(whole));
        } else if (t.site_end > t.site_begin) {
            for (uint64_t g = t.site_begin / 64; g * 64 < t.site_end; ++g) rows += 256ull * wps;
        }
        CHECK(rows == tile_row_bytes_streamed(t, u, wps), "tile %zu: tile_row_bytes_streamed %llu, model %llu", k, (ull)tile_row_bytes_streamed(t, u, wps), (ull)rows);
        bytes += rows + (t.rare_end - t.rare_begin) * 8 + (packed ? single_bytes_streamed(cut.singles[k]) : 0);
    }
    for (uint64_t s = 0; s <= n_rows; ++s) CHECK(read[s] == covered[s], "row %llu is read %u times, covered %u", (ull)s, read[s], covered[s]);
    CHECK(bytes == cut.bytes_streamed, "bytes_streamed %llu, the model's %llu", (ull)cut.bytes_streamed, (ull)bytes);  // 4
    return 0;
}

int main(int argc, char **argv) {
    g_rng = 17;
    if (argc >= 6 && !strcmp(argv[1], "cut")) {
        if ((argc - 6) % 2) return 2;
        const uint32_t tile_blocks = (uint32_t)strtoul(argv[2], nullptr, 10), wps = (uint32_t)strtoul(argv[3], nullptr, 10);
        const uint64_t n_rows = strtoull(argv[4], nullptr, 10);
        std::vector<uint32_t> reps;
        for (const char *p = argv[5]; *p;) {
            char *e;
            reps.push_back((uint32_t)strtoul(p, &e, 10));
            p = *e == ',' ? e + 1 : e;
            if (e == p && *e) return 2;
        }
        if (!tile_blocks || !wps || reps.size() != (n_rows + 63) / 64) return 2;
        for (size_t g = 0; g < reps.size(); ++g) {
            const uint64_t rows = std::min<uint64_t>(64, n_rows - g * 64);
            if (reps[g] < 1 || reps[g] > rows) return 2;
        }
        std::vector<LayoutWindow> w;
        for (int i = 6; i + 1 < argc; i += 2) {
            const uint64_t a = strtoull(argv[i], nullptr, 10), b = strtoull(argv[i + 1], nullptr, 10);
            if (a > b || b > n_rows) return 2;
            w.push_back({{a, 0, 0}, {b, 0, 0}, w.size()});
        }
        TileCut cut;
        if (check_cut(w, tile_blocks, wps, false, n_rows, prefix_of(reps), cut)) return 1;
        std::string split;
        for (size_t k = 0; k < cut.tiles.size(); ++k) {
            const ScanTile &t = cut.tiles[k];
            const UniqRange u = cut.uniqs[k];
            const MidBlocks mb = mid_blocks(t.site_begin, t.site_end);
            split += k ? "," : "";
            if (u.end > u.begin)
                split += std::to_string(mb.g0 * 64 - t.site_begin) + "+" + std::to_string(mb.g1 - mb.g0) + "[" + std::to_string(u.begin) + "-" +
                         std::to_string(u.end) + ")+" + std::to_string(t.site_end - mb.g1 * 64);
            else
                split += std::to_string(t.site_end - t.site_begin) + "+0+0";
        }
        printf("tiles=%zu split=%s bytes=%llu\n", cut.tiles.size(), split.c_str(), (ull)cut.bytes_streamed);
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "random")) {
        g_rng = strtoull(argv[2], nullptr, 10);
        const uint64_t lists = strtoull(argv[3], nullptr, 10);
        static const uint32_t WPS[] = {3, 15, 16}, TB[] = {1, 2, 7, 4096};
        for (uint64_t l = 0; l < lists; ++l) {
            // a matrix of sites, each monomorphic, common (a row), multi or singleton; an edge's three coordinates are the numbers
            // of each kind before it.  Every 16th list: long, tile_blocks 4096 and wps 16, windows that hold thousands of blocks
            const bool big = l % 16 == 15;
            const uint64_t n_site = big ? 64 * (1500 + rnd(2900)) + rnd(64) : 1 + rnd(60 * 64);
            const uint64_t p_mono = big ? 0 : rnd(4) ? rnd(90) : 0, p_rare = big ? rnd(3) : rnd(3) ? rnd(60) : 0, p_single = rnd(101);
            std::vector<EdgeCut> at(n_site + 1);
            EdgeCut run{0, 0, 0};
            for (uint64_t s = 0; s < n_site; ++s) {
                at[s] = run;
                if (rnd(100) < p_mono) continue;
                if (rnd(100) < p_rare) ++(rnd(100) < p_single ? run.g : run.r);
                else ++run.c;
            }
            at[n_site] = run;
            const uint64_t n_rows = run.c;
            // representatives per block: all distinct, all one class, or anything between
            std::vector<uint32_t> reps((n_rows + 63) / 64);
            const uint64_t kind = rnd(4);
            for (size_t g = 0; g < reps.size(); ++g) {
                const uint64_t rows = std::min<uint64_t>(64, n_rows - g * 64);
                reps[g] = kind == 0 ? (uint32_t)rows : kind == 1 ? 1u : 1 + (uint32_t)rnd(rows);
            }
            std::vector<LayoutWindow> w(1 + rnd(big ? 6 : 40));
            for (LayoutWindow &x : w) {
                const uint64_t a = rnd(n_site + 1), room = n_site - a;
                const uint64_t len = rnd(5) == 0 ? 0 : (big || rnd(4) == 0) ? rnd(room + 1) : rnd(std::min<uint64_t>(room, 400) + 1);
                x = {at[a], at[a + len], rnd(1000)};
            }
            if (big) w[0] = {at[rnd(64)], at[n_site - rnd(64)], 0};  // nearly everything: the largest tiles the budget allows
            TileCut cut;
            if (check_cut(w, big ? 4096 : TB[rnd(4)], big ? 16 : WPS[rnd(3)], rnd(2) != 0, n_rows, prefix_of(reps), cut)) {
                fprintf(stderr, "list %llu of seed %s\n", (ull)l, argv[2]);
                return 1;
            }
        }
        printf("random ok lists=%llu\n", (ull)lists);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "bound")) {
        // A tile of tile_blocks <= 4096 at wps 16 touches at most 4097 blocks of rows (tile_cut.cc, property 5), so it holds 0 .. 4097
        // whole blocks.  With a range (1 .. UNIQ_MID_MAX of them) its 64 mid rows stand anywhere in the stream: every offset of the
        // range in its first block and a head or none.  A lane takes one row per block its wave is handed; a representative weighs
        // at most 64 rows of at most 2^16 each; the lane's head or tail row and its rare sites come on top.
        uint64_t worst = 0;
        for (uint64_t mid = 1; mid <= 4097; ++mid) {
            const uint64_t rows = mid * 64;  // as many representatives as rows: no two alike
            uint64_t most = 0;
            for (uint64_t off = 0; off < 64; ++off)
                for (uint64_t head = 0; head < 2; ++head) most = std::max(most, most_mid_blocks_per_wave(head, (off + rows + 63) / 64));
            const uint64_t sum = most * UNIQ_WEIGHT_MAX * UNIQ_ROW_SUM_MAX + UNIQ_ROW_SUM_MAX + UNIQ_RARE_SUM_MAX;
            if (mid <= UNIQ_MID_MAX) {
                CHECK(sum <= uniq_lane_sum_bound(mid), "%llu whole blocks: a lane can reach %llu, uniq_lane_sum_bound says %llu", (ull)mid, (ull)sum,
                      (ull)uniq_lane_sum_bound(mid));
                CHECK(sum < (1ull << 32), "%llu whole blocks: a lane can reach %llu", (ull)mid, (ull)sum);
                worst = std::max(worst, sum);
            } else {
                // no range: rows as they are, at most ceil(4097 / 4) per lane of at most 2^16 each
                CHECK((4097 + 3) / 4 * UNIQ_ROW_SUM_MAX + UNIQ_RARE_SUM_MAX < (1ull << 32), "unweighted rows overflow");
            }
        }
        printf("bound ok worst=%llu\n", (ull)worst);
        return 0;
    }
    return 2;
}
