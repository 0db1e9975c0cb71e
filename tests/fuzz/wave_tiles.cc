// Host check of the one-wave-per-tile condition and rule of csrc/tile_cut.h (plain C++, built with the host sanitizers by
// tests/test_wave_tiles_host.py).
//     wave_tiles bound
//         for every tile size the cap admits (blocks 0 .. WAVE_BLOCKS_MAX; rare words at every value that changes a ceiling near
//         0, 64, ... and near the cap, split between entries and singleton words every way that moves a ceiling) at wps 1 .. 16:
//         the worst lane of a model wave computed here stays <= wave_lane_sum_bound(blocks, rare words) < 2^32, and one step above
//         either cap wave_tile_fits is false.  "bound ok sizes=N worst=X"
//         The model: n = 32 wps haplotypes, the most the width holds.  A lane takes one row of every block, each a representative
//         of weight 64 whose sums are the largest any masks allow — c (n - c) <= floor(n^2 / 4), and the cross term
//         cA (nB - cB) + cB (nA - cA) <= nA nB <= floor(n^2 / 4) — and ceil(E / 64) entries and ceil(W / 64) singleton words, an
//         entry adding the largest m (n - m) or mA (nB - mB) + mB (nA - mA) over m <= 3 and every split of n into nA + nB, found
//         by enumeration, a word four times the same at m = 1.
//     wave_tiles rule N_TILES MAX_BLOCKS MAX_RARE_WORDS N_CU          "wave_tiles=0|1"
//     wave_tiles choice OVERRIDE N_TILES MAX_BLOCKS MAX_RARE_WORDS N_CU   (OVERRIDE -1, 0, 1)   "wave_tiles=0|1"
//     wave_tiles tile SITE_BEGIN SITE_END RARE_BEGIN RARE_END SINGLE_BEGIN SINGLE_END UNIQ_BEGIN UNIQ_END   "blocks=B rare_words=R"
//     wave_tiles random SEED N
//         N random argument tuples: the rule and the forced choice refuse every plan with a tile above the cap; the rule is a pure
//         function (the same answer for the same arguments, whatever was asked between); a plan it takes it also takes with a
//         smaller largest tile or more tiles; override 0 never, override 1 exactly where the cap allows.  "random ok n=N"
// Exit 0, else exit 1 with the breach on stderr.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <set>
#include <vector>

#include "tile_cut.h"

using namespace impop;

#define CHECK(cond, ...)                                                      \
    do {                                                                      \
        if (!(cond)) {                                                        \
            fprintf(stderr, "BREACH %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                                     \
            fprintf(stderr, "\n");                                            \
            exit(1);                                                          \
        }                                                                     \
    } while (0)

// the most one rare site of minor count <= max_m adds to any of a lane's four sums at n haplotypes
static uint64_t worst_rare_site(uint64_t n, uint64_t max_m) {
    uint64_t worst = 0;
    for (uint64_t m = 1; m <= max_m && m < n; ++m) {
        worst = std::max(worst, m * (n - m));
        for (uint64_t nA = 0; nA <= n; ++nA)
            for (uint64_t mA = 0; mA <= m && mA <= nA; ++mA)
                for (uint64_t mB = 0; mA + mB <= m && mB <= n - nA; ++mB)
                    worst = std::max(worst, mA * (n - nA - mB) + mB * (nA - mA));
    }
    return worst;
}

static int run_bound() {
    std::set<uint64_t> rare;
    for (uint64_t base : {(uint64_t)0, (uint64_t)64, (uint64_t)128, (uint64_t)4096, WAVE_RARE_WORDS_MAX / 2, WAVE_RARE_WORDS_MAX})
        for (int64_t d = -66; d <= 66; ++d)
            if ((int64_t)base + d >= 0 && base + d <= WAVE_RARE_WORDS_MAX) rare.insert(base + d);
    uint64_t sizes = 0, worst_seen = 0;
    for (uint32_t wps = 1; wps <= 16; ++wps) {
        const uint64_t n = 32ull * wps, row = (n * n / 4) * UNIQ_WEIGHT_MAX;
        CHECK(n * n / 4 <= UNIQ_ROW_SUM_MAX, "wps %u", wps);
        const uint64_t entry = worst_rare_site(n, 3), word = 4 * worst_rare_site(n, 1);
        CHECK(entry <= WAVE_RARE_SITE_SUM_MAX && word <= WAVE_RARE_WORD_SUM_MAX, "wps %u: entry %llu word %llu", wps,
              (unsigned long long)entry, (unsigned long long)word);
        for (uint64_t blocks = 0; blocks <= WAVE_BLOCKS_MAX; ++blocks)
            for (uint64_t rw : rare) {
                CHECK(wave_tile_fits(blocks, rw), "%llu %llu", (unsigned long long)blocks, (unsigned long long)rw);
                const uint64_t bound = wave_lane_sum_bound(blocks, rw);
                CHECK(bound < (1ull << 32), "bound %llu at %llu blocks %llu rare words", (unsigned long long)bound,
                      (unsigned long long)blocks, (unsigned long long)rw);
                // entries E and singleton words W = rw - E: all of one kind, halves, and the splits that leave one word past a 64
                for (uint64_t E : {(uint64_t)0, rw, rw / 2, rw > 0 ? (uint64_t)1 : 0, rw >= 65 ? (uint64_t)65 : rw, rw - std::min<uint64_t>(rw, 1),
                                   rw - std::min<uint64_t>(rw, 65)}) {
                    const uint64_t W = rw - E;
                    const uint64_t lane = blocks * row + ((E + 63) / 64) * entry + ((W + 63) / 64) * word;
                    CHECK(lane <= bound, "wps %u: lane %llu > bound %llu at %llu blocks, %llu entries, %llu words", wps,
                          (unsigned long long)lane, (unsigned long long)bound, (unsigned long long)blocks, (unsigned long long)E,
                          (unsigned long long)W);
                    worst_seen = std::max(worst_seen, lane);
                    ++sizes;
                }
            }
    }
    CHECK(!wave_tile_fits(WAVE_BLOCKS_MAX + 1, 0) && !wave_tile_fits(0, WAVE_RARE_WORDS_MAX + 1), "one above the cap fits");
    printf("bound ok sizes=%llu worst=%llu\n", (unsigned long long)sizes, (unsigned long long)worst_seen);
    return 0;
}

static uint64_t rnd(uint64_t &s) {
    s += 0x9E3779B97F4A7C15ull;
    uint64_t x = s;
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

static int run_random(uint64_t seed, uint64_t count) {
    struct Args { uint64_t tiles, blocks, rare; int cu; bool rule; };
    std::vector<Args> asked;
    uint64_t s = seed;
    for (uint64_t i = 0; i < count; ++i) {
        Args a;
        // sizes around the thresholds, around the caps, and anywhere
        const uint64_t kind = rnd(s) % 4;
        a.blocks = kind == 0 ? rnd(s) % (2 * WAVE_RULE_BLOCKS + 2) : kind == 1 ? WAVE_BLOCKS_MAX - 2 + rnd(s) % 5 : rnd(s) % 5000;
        a.rare = kind == 0 ? rnd(s) % (2 * WAVE_RULE_RARE_WORDS + 2) : kind == 2 ? WAVE_RARE_WORDS_MAX - 2 + rnd(s) % 5 : rnd(s) % (1ull << 22);
        a.cu = (int)(rnd(s) % 5 == 0 ? 0 : 1 + rnd(s) % 400);
        const uint64_t cu = a.cu > 0 ? (uint64_t)a.cu : 256;
        a.tiles = rnd(s) % 3 == 0 ? WAVE_RULE_TILES_PER_CU * cu - 1 + rnd(s) % 3 : rnd(s) % (4 * WAVE_RULE_TILES_PER_CU * cu);
        a.rule = wave_tile_rule(a.tiles, a.blocks, a.rare, a.cu);
        const bool fits = wave_tile_fits(a.blocks, a.rare);
        CHECK(fits == (a.blocks <= WAVE_BLOCKS_MAX && a.rare <= WAVE_RARE_WORDS_MAX), "fits");
        if (!fits) {
            CHECK(!a.rule, "the rule takes a plan above the cap: %llu blocks %llu rare words", (unsigned long long)a.blocks, (unsigned long long)a.rare);
            CHECK(!wave_tile_choice(1, a.tiles, a.blocks, a.rare, a.cu) && !wave_tile_choice(-1, a.tiles, a.blocks, a.rare, a.cu), "forced above the cap");
        }
        CHECK(!wave_tile_choice(0, a.tiles, a.blocks, a.rare, a.cu), "override 0");
        CHECK(wave_tile_choice(1, a.tiles, a.blocks, a.rare, a.cu) == fits, "override 1");
        CHECK(wave_tile_choice(-1, a.tiles, a.blocks, a.rare, a.cu) == a.rule, "no override");
        if (a.rule) {
            CHECK(a.tiles >= WAVE_RULE_TILES_PER_CU * cu, "the rule takes %llu tiles on %llu CUs", (unsigned long long)a.tiles, (unsigned long long)cu);
            CHECK(wave_tile_rule(a.tiles + 1 + rnd(s) % 1000, a.blocks - rnd(s) % (a.blocks + 1), a.rare - rnd(s) % (a.rare + 1), a.cu),
                  "not monotonic");
        }
        asked.push_back(a);
    }
    for (size_t i = asked.size(); i-- > 0;) {  // asked again, in another order: the same answers
        const Args &a = asked[i];
        CHECK(wave_tile_rule(a.tiles, a.blocks, a.rare, a.cu) == a.rule, "the rule changed its answer");
    }
    printf("random ok n=%llu\n", (unsigned long long)count);
    return 0;
}

int main(int argc, char **argv) {
    auto num = [&](int i) { return strtoull(argv[i], nullptr, 10); };
    if (argc == 2 && !strcmp(argv[1], "bound")) return run_bound();
    if (argc == 4 && !strcmp(argv[1], "random")) return run_random(num(2), num(3));
    if (argc == 6 && !strcmp(argv[1], "rule")) {
        printf("wave_tiles=%d\n", (int)wave_tile_rule(num(2), num(3), num(4), atoi(argv[5])));
        return 0;
    }
    if (argc == 7 && !strcmp(argv[1], "choice")) {
        printf("wave_tiles=%d\n", (int)wave_tile_choice(atoi(argv[2]), num(3), num(4), num(5), atoi(argv[6])));
        return 0;
    }
    if (argc == 10 && !strcmp(argv[1], "tile")) {
        const ScanTile t{num(2), num(3), num(4), num(5)};
        printf("blocks=%llu rare_words=%llu\n", (unsigned long long)tile_blocks_read(t, UniqRange{num(8), num(9)}),
               (unsigned long long)tile_rare_words(t, SingleRange{num(6), num(7)}));
        return 0;
    }
    fprintf(stderr, "usage: wave_tiles bound | random SEED N | rule ... | choice ... | tile ...\n");
    return 2;
}
