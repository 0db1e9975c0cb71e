// Host check of csrc/win_chunks.h (plain C++, built with the host sanitizers by tests/test_win_chunks_host.py).
//     win_chunks plan BUDGET CAP N_TILES PER_TILE PER_WIN PER_ITEM  t0 t1  t0 t1 ...
//         plans the windows (tile ranges [t0, t1); t0 == t1: a window without tiles; CAP 0: no cap) and checks the plan against a
//         brute-force model computed here from sets of tiles.  One line: "chunks=K sizes=a,b,..." (windows per chunk).
//     win_chunks random SEED LISTS
//         the same check on LISTS seeded random lists of at most 40 windows over at most 60 tiles.  "random ok lists=N"
//     win_chunks members
//         the member set on n_hap in {1, 31, 32, 33, 64, 65, 465}.  "members ok cases=N"
// Exit 0, else exit 1 with the breached property on stderr.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <string>
#include <vector>

#include "win_chunks.h"

struct Win {
    uint64_t t0, t1;
};

#define CHECK(cond, ...)                                                      \
    do {                                                                      \
        if (!(cond)) {                                                        \
            fprintf(stderr, "BREACH %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                                     \
            fprintf(stderr, "\n");                                            \
            return 1;                                                         \
        }                                                                     \
    } while (0)

// the model: the bytes of windows [b, e) as one chunk — every tile any of them holds once, every window, every (window, tile)
static uint64_t model_bytes(const std::vector<Win> &w, uint64_t b, uint64_t e, const impop::TileCosts &k) {
    std::set<uint64_t> tiles;
    uint64_t items = 0;
    for (uint64_t i = b; i < e; ++i)
        for (uint64_t t = w[i].t0; t < w[i].t1; ++t) {
            tiles.insert(t);
            ++items;
        }
    return tiles.size() * k.per_tile + (e - b) * k.per_win + items * k.per_item;
}

static int check_plan(const std::vector<Win> &w, uint64_t n_tiles, uint64_t budget, uint64_t cap, const impop::TileCosts &k,
                      std::string *sizes) {
    const uint64_t n = w.size();
    const std::vector<impop::TiledChunk> plan = impop::plan_tiled_chunks(w.data(), n, n_tiles, budget, cap, k);
    CHECK((n == 0) == plan.empty(), "%zu chunks for %llu windows", plan.size(), (unsigned long long)n);
    uint64_t next = 0;
    for (size_t c = 0; c < plan.size(); ++c) {
        const impop::TiledChunk &ch = plan[c];
        CHECK(ch.w_begin == next && ch.w_end > ch.w_begin && ch.w_end <= n, "chunk %zu is [%llu, %llu) after %llu windows", c,
              (unsigned long long)ch.w_begin, (unsigned long long)ch.w_end, (unsigned long long)next);
        next = ch.w_end;
        const uint64_t cnt = ch.w_end - ch.w_begin;
        CHECK(!cap || cnt <= cap, "chunk %zu holds %llu windows, cap %llu", c, (unsigned long long)cnt, (unsigned long long)cap);
        std::set<uint64_t> want;
        uint64_t items = 0;
        for (uint64_t i = ch.w_begin; i < ch.w_end; ++i)
            for (uint64_t t = w[i].t0; t < w[i].t1; ++t) {
                want.insert(t);
                ++items;
            }
        CHECK(ch.tiles.size() == want.size() && ch.items == items, "chunk %zu: %zu tiles / %llu items, model %zu / %llu", c, ch.tiles.size(),
              (unsigned long long)ch.items, want.size(), (unsigned long long)items);
        for (size_t j = 0; j < ch.tiles.size(); ++j) {
            CHECK(j == 0 || ch.tiles[j - 1] < ch.tiles[j], "chunk %zu: tiles not strictly ascending at %zu", c, j);
            CHECK(want.count(ch.tiles[j]) == 1, "chunk %zu: tile %llu belongs to none of its windows", c, (unsigned long long)ch.tiles[j]);
        }
        CHECK(ch.l0.size() == cnt, "chunk %zu: %zu first tiles for %llu windows", c, ch.l0.size(), (unsigned long long)cnt);
        for (uint64_t i = ch.w_begin; i < ch.w_end; ++i) {
            const uint32_t l0 = ch.l0[i - ch.w_begin];
            if (w[i].t1 == w[i].t0) CHECK(l0 == 0, "chunk %zu: window %llu has no tiles and l0 = %u", c, (unsigned long long)i, l0);
            CHECK(l0 + (w[i].t1 - w[i].t0) <= ch.tiles.size(), "chunk %zu: window %llu reads past the chunk's tiles", c, (unsigned long long)i);
            for (uint64_t j = 0; j < w[i].t1 - w[i].t0; ++j)
                CHECK(ch.tiles[l0 + j] == w[i].t0 + j, "chunk %zu: window %llu: local tile %llu is %llu, not %llu", c, (unsigned long long)i,
                      (unsigned long long)(l0 + j), (unsigned long long)ch.tiles[l0 + j], (unsigned long long)(w[i].t0 + j));
        }
        const uint64_t bytes = model_bytes(w, ch.w_begin, ch.w_end, k);
        CHECK(bytes <= budget || cnt == 1, "chunk %zu: %llu bytes of %llu windows against a budget of %llu", c, (unsigned long long)bytes,
              (unsigned long long)cnt, (unsigned long long)budget);
        if (c + 1 < plan.size())
            CHECK(model_bytes(w, ch.w_begin, ch.w_end + 1, k) > budget || (cap && cnt == cap),
                  "chunk %zu stopped at %llu windows although the next one fits", c, (unsigned long long)cnt);
        if (sizes) *sizes += (c ? "," : "") + std::to_string(cnt);
    }
    CHECK(next == n, "the chunks hold %llu of %llu windows", (unsigned long long)next, (unsigned long long)n);

    // the untiled cutter on the same list, a window's bytes its tile count: the same properties, from plain sums
    const std::vector<impop::WinChunk> cuts =
        impop::cut_windows(n, budget, cap, [&](size_t, uint64_t i) { return k.per_win + (w[i].t1 - w[i].t0) * k.per_item; });
    next = 0;
    for (size_t c = 0; c < cuts.size(); ++c) {
        CHECK(cuts[c].w_begin == next && cuts[c].w_end > next && cuts[c].w_end <= n, "cut %zu is out of order", c);
        next = cuts[c].w_end;
        const uint64_t cnt = cuts[c].w_end - cuts[c].w_begin;
        uint64_t bytes = 0;
        for (uint64_t i = cuts[c].w_begin; i < cuts[c].w_end; ++i) bytes += k.per_win + (w[i].t1 - w[i].t0) * k.per_item;
        CHECK((bytes <= budget || cnt == 1) && (!cap || cnt <= cap), "cut %zu: %llu bytes, %llu windows", c, (unsigned long long)bytes,
              (unsigned long long)cnt);
        if (c + 1 < cuts.size())
            CHECK(bytes + k.per_win + (w[next].t1 - w[next].t0) * k.per_item > budget || (cap && cnt == cap), "cut %zu stopped early", c);
    }
    CHECK(next == n, "the cuts hold %llu of %llu windows", (unsigned long long)next, (unsigned long long)n);
    return 0;
}

static uint64_t g_rng;
static uint64_t rnd(uint64_t below) {  // splitmix64
    uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (z ^ (z >> 31)) % below;
}

static int check_members(uint32_t n_hap, const std::vector<uint64_t> *mask, const std::vector<uint8_t> &in) {
    const uint32_t wps = (n_hap + 31) / 32;
    const impop::MemberSet s = impop::member_set(mask ? mask->data() : nullptr, n_hap, wps);
    CHECK(s.ppos.size() == (size_t)wps * 32 && s.bits.size() == wps, "n_hap %u: table sizes", n_hap);
    uint32_t members = 0, pop = 0;
    for (uint32_t i = 0; i < wps * 32; ++i) {
        const bool is = i < n_hap && in[i];
        CHECK(((s.bits[i >> 5] >> (i & 31)) & 1u) == (is ? 1u : 0u), "n_hap %u: bit %u", n_hap, i);
        if (is) {
            CHECK(members < s.idx.size() && s.idx[members] == i && s.ppos[i] == (int32_t)members, "n_hap %u: member %u is not idx[%u]", n_hap, i, members);
            ++members;
        } else {
            CHECK(s.ppos[i] == -1, "n_hap %u: ppos[%u] = %d for a non-member", n_hap, i, s.ppos[i]);
        }
    }
    for (uint32_t d : s.bits) pop += (uint32_t)__builtin_popcount(d);
    CHECK(members == s.idx.size() && pop == members && s.size() == members, "n_hap %u: %u members, idx holds %zu, %u bits", n_hap, members,
          s.idx.size(), pop);
    for (size_t j = 1; j < s.idx.size(); ++j) CHECK(s.idx[j - 1] < s.idx[j], "n_hap %u: idx not ascending at %zu", n_hap, j);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "plan")) {
        if (argc < 8 || (argc - 8) % 2) return 2;
        const uint64_t budget = strtoull(argv[2], nullptr, 10), cap = strtoull(argv[3], nullptr, 10), n_tiles = strtoull(argv[4], nullptr, 10);
        const impop::TileCosts k{strtoull(argv[5], nullptr, 10), strtoull(argv[6], nullptr, 10), strtoull(argv[7], nullptr, 10)};
        std::vector<Win> w;
        for (int i = 8; i + 1 < argc; i += 2) {
            w.push_back({strtoull(argv[i], nullptr, 10), strtoull(argv[i + 1], nullptr, 10)});
            if (w.back().t1 < w.back().t0 || w.back().t1 > n_tiles) return 2;
        }
        std::string sizes;
        if (check_plan(w, n_tiles, budget, cap, k, &sizes)) return 1;
        printf("chunks=%zu sizes=%s\n", (size_t)std::count(sizes.begin(), sizes.end(), ',') + (sizes.empty() ? 0 : 1), sizes.c_str());
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "random")) {
        g_rng = strtoull(argv[2], nullptr, 10);
        const uint64_t lists = strtoull(argv[3], nullptr, 10);
        for (uint64_t l = 0; l < lists; ++l) {
            const uint64_t n_tiles = 1 + rnd(60), n = 1 + rnd(40);
            std::vector<Win> w(n);
            for (Win &x : w) {
                x.t0 = rnd(n_tiles + 1);
                x.t1 = rnd(4) == 0 ? x.t0 : x.t0 + rnd(std::min<uint64_t>(n_tiles - x.t0, 12) + 1);
            }
            const impop::TileCosts k{1 + rnd(100), rnd(50), rnd(3) ? rnd(9) : 0};
            const uint64_t all = model_bytes(w, 0, n, k);
            const uint64_t budget = rnd(5) == 0 ? all : 1 + rnd(all + 1), cap = rnd(3) == 0 ? 1 + rnd(6) : 0;
            if (check_plan(w, n_tiles, budget, cap, k, nullptr)) {
                fprintf(stderr, "list %llu of seed %s\n", (unsigned long long)l, argv[2]);
                return 1;
            }
        }
        printf("random ok lists=%llu\n", (unsigned long long)lists);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "members")) {
        g_rng = 20240607;
        int cases = 0;
        for (uint32_t n_hap : {1u, 31u, 32u, 33u, 64u, 65u, 465u}) {
            const uint32_t words = (n_hap + 63) / 64;
            for (int kind = 0; kind < 5; ++kind, ++cases) {  // null, empty, first only, last only, random
                std::vector<uint8_t> in(n_hap, kind == 0);
                if (kind == 2) in[0] = 1;
                if (kind == 3) in[n_hap - 1] = 1;
                if (kind == 4)
                    for (uint8_t &b : in) b = (uint8_t)rnd(2);
                std::vector<uint64_t> mask(words, 0);
                for (uint32_t i = 0; i < n_hap; ++i) mask[i >> 6] |= (uint64_t)in[i] << (i & 63);
                for (uint32_t i = n_hap; i < words * 64; ++i) mask[i >> 6] |= 1ull << (i & 63);  // the spare bits: all set, to be ignored
                if (check_members(n_hap, kind == 0 ? nullptr : &mask, in)) return 1;
            }
        }
        printf("members ok cases=%d\n", cases);
        return 0;
    }
    return 2;
}
