// Host check of csrc/tile_cut.h (plain C++, built with the host sanitizers by tests/test_tile_cut_host.py).
//     tile_cut cut TILE_BLOCKS WPS PACKED  c0 r0 g0 c1 r1 g1  ...
//         cuts the windows (six numbers each: the low and the high edge as site of the layout, rare entry, singleton) and checks
//         the cut against a model computed here from the covered indices of each stream.  One line: "tiles=K sizes=a,b,..." with a
//         tile as its blocks touched, or blocks+entries+singletons where it has rare sites.
//     tile_cut random SEED LISTS
//         the same check on LISTS seeded random lists of at most 40 windows over at most 60 blocks of sites.  "random ok lists=N"
//     tile_cut rule WPS BLOCKS N_CU
//         default_tile_rule.  "tile_blocks=N"
// Properties (every cut, packed or not):
//   1 within each stream the tiles' ranges are ascending and disjoint and their union is exactly what the windows cover
//   2 a non-empty window's tiles [t0, t1) cover exactly its range in each stream; a window empty in all three has t0 == t1
//   3 no tile is empty in all three streams
//   4 a tile's site range starts and ends on a multiple of 64 or on a window edge
//   5 a tile touches blocks and holds rare sites worth at most budget + row_bytes + 8 bytes (n_parts = ceil(total / budget) and the
//     two ceilings per, per_r), and at most budget / 8 rare sites (per_r <= ceil(nr / (8 nr / budget)) and 8 | budget): 2^21 at
//     tile_blocks = 4096 and wps <= 16, which the fixed-WPS kernel's 32-bit lane accumulators rest on
//   6 packed against split: the cut of the same windows with the singletons folded into the entries, r' = r + g, has the same
//     tiles by number and site range, the same (t0, t1) per window, and per tile as many entries as entries + singletons
//   7 bytes_streamed is the sum of tile_bytes_streamed and single_bytes_streamed over the output
//   8 permuting the windows permutes wins and changes neither the tiles nor bytes_streamed
// Exit 0, else exit 1 with the breached property on stderr.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
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

struct Range {
    uint64_t b, e;
};
// stream 0: sites, 1: entries of the rare stream, 2: singletons
static Range win_range(const LayoutWindow &w, int s) {
    return s == 0 ? Range{w.lo.c, w.hi.c} : s == 1 ? Range{w.lo.r, w.hi.r} : Range{w.lo.g, w.hi.g};
}
static Range tile_range(const TileCut &t, size_t k, int s) {
    if (s == 0) return {t.tiles[k].site_begin, t.tiles[k].site_end};
    if (s == 1) return {t.tiles[k].rare_begin, t.tiles[k].rare_end};
    return t.singles.empty() ? Range{0, 0} : Range{t.singles[k].begin, t.singles[k].end};
}

static int check_one(const std::vector<LayoutWindow> &w, uint32_t tile_blocks, uint32_t wps, bool packed, TileCut &cut) {
    cut = TileCut();
    cut_tiles(w, tile_blocks, wps, packed, cut);
    const size_t nt = cut.tiles.size();
    CHECK(cut.wins.size() == w.size() && cut.singles.size() == (packed ? nt : 0), "%zu wins for %zu windows, %zu singles for %zu tiles",
          cut.wins.size(), w.size(), cut.singles.size(), nt);
    std::set<uint64_t> edges;
    for (const LayoutWindow &x : w)
        if (!x.empty()) {
            edges.insert(x.lo.c);
            edges.insert(x.hi.c);
        }
    for (int s = 0; s < 3; ++s) {
        uint64_t top = 0;
        for (const LayoutWindow &x : w) top = std::max(top, win_range(x, s).e);
        std::vector<uint32_t> covered(top + 1, 0), read(top + 1, 0);  // the model: which indices some window holds
        for (const LayoutWindow &x : w)
            for (uint64_t i = win_range(x, s).b; i < win_range(x, s).e; ++i) covered[i] = 1;
        uint64_t last = 0;
        for (size_t k = 0; k < nt; ++k) {  // 1
            const Range r = tile_range(cut, k, s);
            CHECK(r.b <= r.e && r.e <= top, "stream %d: tile %zu is [%llu, %llu) of %llu", s, k, (ull)r.b, (ull)r.e, (ull)top);
            if (r.b == r.e) continue;
            CHECK(r.b >= last, "stream %d: tile %zu starts at %llu before %llu", s, k, (ull)r.b, (ull)last);
            last = r.e;
            for (uint64_t i = r.b; i < r.e; ++i) ++read[i];
        }
        for (uint64_t i = 0; i <= top; ++i)
            CHECK(read[i] == covered[i], "stream %d: index %llu is read %u times, covered %u", s, (ull)i, read[i], covered[i]);
        for (size_t i = 0; i < w.size(); ++i) {  // 2
            const WinDesc &d = cut.wins[i];
            const Range want = win_range(w[i], s);
            CHECK(d.t0 <= d.t1 && d.t1 <= nt, "window %zu: tiles [%llu, %llu) of %zu", i, (ull)d.t0, (ull)d.t1, nt);
            if (w[i].empty()) CHECK(d.t0 == d.t1, "window %zu is empty and has tiles", i);
            uint64_t len = 0;
            for (uint64_t k = d.t0; k < d.t1; ++k) {
                const Range r = tile_range(cut, k, s);
                if (r.b == r.e) continue;
                CHECK(r.b >= want.b && r.e <= want.e, "stream %d: window %zu [%llu, %llu): its tile %llu is [%llu, %llu)", s, i, (ull)want.b,
                      (ull)want.e, (ull)k, (ull)r.b, (ull)r.e);
                len += r.e - r.b;
            }
            CHECK(len == want.e - want.b, "stream %d: window %zu: its tiles hold %llu of %llu", s, i, (ull)len, (ull)(want.e - want.b));
        }
    }
    const uint64_t row_bytes = 256ull * wps, budget = (uint64_t)tile_blocks * row_bytes;
    uint64_t bytes = 0;
    for (size_t k = 0; k < nt; ++k) {
        const ScanTile &t = cut.tiles[k];
        const Range g = tile_range(cut, k, 2);
        const uint64_t nr = (t.rare_end - t.rare_begin) + (g.e - g.b);
        const uint64_t blocks = t.site_end > t.site_begin ? (t.site_end + 63) / 64 - t.site_begin / 64 : 0;
        CHECK(blocks || nr, "tile %zu is empty", k);  // 3
        if (blocks) {                                  // 4
            CHECK(t.site_begin % 64 == 0 || edges.count(t.site_begin), "tile %zu starts at site %llu", k, (ull)t.site_begin);
            CHECK(t.site_end % 64 == 0 || edges.count(t.site_end), "tile %zu ends at site %llu", k, (ull)t.site_end);
        }
        CHECK(blocks * row_bytes + 8 * nr <= budget + row_bytes + 8, "tile %zu: %llu blocks and %llu rare sites against %llu bytes", k,  // 5
              (ull)blocks, (ull)nr, (ull)budget);
        CHECK(nr <= budget / 8, "tile %zu: %llu rare sites, budget / 8 = %llu", k, (ull)nr, (ull)(budget / 8));
        if (tile_blocks == 4096 && wps <= 16) CHECK(nr <= (1ull << 21), "tile %zu: %llu rare sites", k, (ull)nr);
        bytes += tile_bytes_streamed(t, wps) + (packed ? single_bytes_streamed(cut.singles[k]) : 0);
    }
    CHECK(bytes == cut.bytes_streamed, "bytes_streamed %llu, the tiles add up to %llu", (ull)cut.bytes_streamed, (ull)bytes);  // 7
    return 0;
}

static uint64_t g_rng;
static uint64_t rnd(uint64_t below) {  // splitmix64
    uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (z ^ (z >> 31)) % below;
}

static bool same_tiles(const TileCut &a, const TileCut &b, bool rare_too) {
    if (a.tiles.size() != b.tiles.size() || a.singles.size() != (rare_too ? b.singles.size() : a.singles.size())) return false;
    for (size_t k = 0; k < a.tiles.size(); ++k) {
        if (a.tiles[k].site_begin != b.tiles[k].site_begin || a.tiles[k].site_end != b.tiles[k].site_end) return false;
        if (rare_too && (a.tiles[k].rare_begin != b.tiles[k].rare_begin || a.tiles[k].rare_end != b.tiles[k].rare_end)) return false;
        if (rare_too && !a.singles.empty() && (a.singles[k].begin != b.singles[k].begin || a.singles[k].end != b.singles[k].end)) return false;
    }
    return true;
}

static int check_cut(const std::vector<LayoutWindow> &w, uint32_t tile_blocks, uint32_t wps, bool packed, TileCut &cut) {
    if (check_one(w, tile_blocks, wps, packed, cut)) return 1;
    // 8: a permutation of the windows (a seeded shuffle; seq_len carries the window's place in the original list)
    std::vector<LayoutWindow> p = w;
    for (size_t i = 0; i < p.size(); ++i) p[i].seq_len = i;
    for (size_t i = p.size(); i > 1; --i) std::swap(p[i - 1], p[rnd(i)]);
    TileCut pc;
    if (check_one(p, tile_blocks, wps, packed, pc)) return 1;
    CHECK(same_tiles(cut, pc, true) && cut.bytes_streamed == pc.bytes_streamed, "a permutation of the windows changes the tiles");
    for (size_t i = 0; i < p.size(); ++i) {
        const WinDesc &a = pc.wins[i], &b = cut.wins[p[i].seq_len];
        CHECK(a.t0 == b.t0 && a.t1 == b.t1 && a.n_sites == b.n_sites && a.seq_len == p[i].seq_len, "window %llu moved to %zu: [%llu, %llu) was [%llu, %llu)",
              (ull)p[i].seq_len, i, (ull)a.t0, (ull)a.t1, (ull)b.t0, (ull)b.t1);
    }
    if (!packed) return 0;
    // 6: the split route's cut of the same windows
    std::vector<LayoutWindow> f = w;
    for (LayoutWindow &x : f) {
        x.lo = {x.lo.c, x.lo.r + x.lo.g, 0};
        x.hi = {x.hi.c, x.hi.r + x.hi.g, 0};
    }
    TileCut fc;
    if (check_one(f, tile_blocks, wps, false, fc)) return 1;
    CHECK(same_tiles(cut, fc, false), "packed: %zu tiles, split: %zu, or their site ranges differ", cut.tiles.size(), fc.tiles.size());
    for (size_t i = 0; i < w.size(); ++i)
        CHECK(cut.wins[i].t0 == fc.wins[i].t0 && cut.wins[i].t1 == fc.wins[i].t1, "window %zu: packed tiles [%llu, %llu), split [%llu, %llu)", i,
              (ull)cut.wins[i].t0, (ull)cut.wins[i].t1, (ull)fc.wins[i].t0, (ull)fc.wins[i].t1);
    for (size_t k = 0; k < cut.tiles.size(); ++k)
        CHECK(fc.tiles[k].rare_end - fc.tiles[k].rare_begin ==
                  (cut.tiles[k].rare_end - cut.tiles[k].rare_begin) + (cut.singles[k].end - cut.singles[k].begin),
              "tile %zu: split holds %llu entries, packed %llu + %llu", k, (ull)(fc.tiles[k].rare_end - fc.tiles[k].rare_begin),
              (ull)(cut.tiles[k].rare_end - cut.tiles[k].rare_begin), (ull)(cut.singles[k].end - cut.singles[k].begin));
    return 0;
}

int main(int argc, char **argv) {
    g_rng = 17;
    if (argc >= 5 && !strcmp(argv[1], "cut")) {
        if ((argc - 5) % 6) return 2;
        const uint32_t tile_blocks = (uint32_t)strtoul(argv[2], nullptr, 10), wps = (uint32_t)strtoul(argv[3], nullptr, 10);
        const bool packed = strtoul(argv[4], nullptr, 10) != 0;
        std::vector<LayoutWindow> w;
        for (int i = 5; i + 5 < argc; i += 6) {
            uint64_t v[6];
            for (int j = 0; j < 6; ++j) v[j] = strtoull(argv[i + j], nullptr, 10);
            if (v[3] < v[0] || v[4] < v[1] || v[5] < v[2] || !tile_blocks || !wps) return 2;
            w.push_back({{v[0], v[1], v[2]}, {v[3], v[4], v[5]}, w.size()});
        }
        TileCut cut;
        if (check_cut(w, tile_blocks, wps, packed, cut)) return 1;
        std::string sizes;
        for (size_t k = 0; k < cut.tiles.size(); ++k) {
            const ScanTile &t = cut.tiles[k];
            const uint64_t m = t.rare_end - t.rare_begin, g = packed ? cut.singles[k].end - cut.singles[k].begin : 0;
            sizes += (k ? "," : "") + std::to_string(t.site_end > t.site_begin ? (t.site_end + 63) / 64 - t.site_begin / 64 : 0);
            if (m || g) sizes += "+" + std::to_string(m) + "+" + std::to_string(g);
        }
        printf("tiles=%zu sizes=%s\n", cut.tiles.size(), sizes.c_str());
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "random")) {
        g_rng = strtoull(argv[2], nullptr, 10);
        const uint64_t lists = strtoull(argv[3], nullptr, 10);
        static const uint32_t WPS[] = {1, 3, 15, 16, 40}, TB[] = {1, 2, 7, 4096};
        for (uint64_t l = 0; l < lists; ++l) {
            // a matrix of sites, each monomorphic (in no stream), common, multi or singleton: the three coordinates of an edge are
            // the numbers of each kind before it, monotone maps of the site as the index produces them.
            // kind 0: a mix; 1: no rare sites at all; 2: rare sites only; 3: every rare site a singleton
            const uint64_t n_site = 1 + rnd(60 * 64), kind = rnd(6) < 3 ? 0 : 1 + rnd(3);
            const uint64_t p_mono = rnd(4) ? rnd(90) : 0, p_rare = kind == 1 ? 0 : kind == 2 ? 100 : rnd(101),
                           p_single = kind == 3 ? 100 : rnd(101);
            std::vector<EdgeCut> at(n_site + 1);
            EdgeCut run{0, 0, 0};
            for (uint64_t s = 0; s < n_site; ++s) {
                at[s] = run;
                if (rnd(100) < p_mono) continue;
                if (rnd(100) < p_rare) ++(rnd(100) < p_single ? run.g : run.r);
                else ++run.c;
            }
            at[n_site] = run;
            std::vector<LayoutWindow> w(1 + rnd(40));
            for (LayoutWindow &x : w) {
                const uint64_t a = rnd(n_site + 1), room = n_site - a;
                const uint64_t len = rnd(5) == 0 ? 0 : rnd(4) == 0 ? rnd(room + 1) : rnd(std::min<uint64_t>(room, 400) + 1);
                x = {at[a], at[a + len], rnd(1000)};
            }
            TileCut cut;
            if (check_cut(w, TB[rnd(4)], WPS[rnd(5)], true, cut)) {
                fprintf(stderr, "list %llu of seed %s\n", (ull)l, argv[2]);
                return 1;
            }
        }
        printf("random ok lists=%llu\n", (ull)lists);
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "rule")) {
        printf("tile_blocks=%u\n", default_tile_rule((uint32_t)strtoul(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10), atoi(argv[4])));
        return 0;
    }
    return 2;
}
