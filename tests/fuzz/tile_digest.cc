// Host check of csrc/tile_digest.h (plain C++, built with the host sanitizers by tests/test_tile_digest_host.py): what a digest
// tile may hold, when a plan takes the digest, and where every tile's share of it lies.
//     tile_digest bound
//         for wps 1 .. 16 and tile sizes up to the caps (common rows, singletons and entries at every value that changes a ceiling
//         near 0, 64, ... and at the caps): the worst lane of a model wave stays <= digest_lane_sum_bound(...) < 2^32, and one step
//         above any cap digest_tile_fits is false.  "bound ok sizes=N worst=X"
//         The model: n = 32 wps haplotypes.  A lane may hold EVERY common row of the tile (weights are free: one representative may
//         stand for all of them), each adding the largest c (n - c) or cross term, floor(n^2 / 4); every singleton, through the
//         histogram (all on one haplotype's lane: k (n_X - 1) or n_B k_A + n_A k_B - 2 k_AB, at most k n), or, where the tile keeps
//         its range, one in 64 of its words, rounded up twice for the two ends; and one in 64 of the entries, rounded up.
//     tile_digest fits CANDIDATES COMMON_ROWS SINGLES ENTRIES                      "fits=0|1"
//     tile_digest candidates SITE_BEGIN SITE_END UNIQ_BEGIN UNIQ_END               "candidates=N"
//     tile_digest hist SINGLE_BEGIN SINGLE_END WPS                                 "hist=0|1"
//     tile_digest choice OVERRIDE REUSABLE WAVE_TILES ALL_FIT DIGEST_BYTES PLAIN_BYTES   "digest=0|1"
//     tile_digest random SEED N
//         N random tile lists: per-tile offsets, sizes and alignment of the layout, no overlap, digest_bytes the sum over tiles,
//         bytes_streamed the sum of what every tile reads; the rule never takes a plan that reads more with the digest than without,
//         never a one-shot plan, never one with a tile above the caps; override 0 never, override 1 exactly where the body is the
//         one-wave one and every tile fits.  "random ok n=N"
// Exit 0, else exit 1 with the breach on stderr.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <set>
#include <vector>

#include "tile_digest.h"

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
typedef unsigned long long ull;

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

static std::set<uint64_t> around(std::initializer_list<uint64_t> bases, uint64_t cap) {
    std::set<uint64_t> out;
    for (uint64_t b : bases)
        for (int64_t d = -66; d <= 66; ++d)
            if ((int64_t)b + d >= 0 && b + d <= cap) out.insert(b + d);
    return out;
}

static int run_bound() {
    const std::set<uint64_t> rows = around({0, 64, 512, DIGEST_COMMON_MAX / 2, DIGEST_COMMON_MAX}, DIGEST_COMMON_MAX);
    const std::set<uint64_t> singles = around({0, 256, 4096, DIGEST_SINGLES_MAX}, DIGEST_SINGLES_MAX);
    const std::set<uint64_t> entries = {0, 1, 63, 64, 65, 4096, WAVE_RARE_WORDS_MAX - 1, WAVE_RARE_WORDS_MAX};
    uint64_t sizes = 0, worst_seen = 0;
    for (uint32_t wps = 1; wps <= 16; ++wps) {
        const uint64_t n = 32ull * wps, row = n * n / 4;
        CHECK(row <= UNIQ_ROW_SUM_MAX, "wps %u", wps);
        const uint64_t entry = worst_rare_site(n, 3), one = worst_rare_site(n, 1);
        CHECK(entry <= WAVE_RARE_SITE_SUM_MAX && one <= DIGEST_SINGLE_SUM_MAX && 4 * one <= WAVE_RARE_WORD_SUM_MAX, "wps %u: entry %llu single %llu",
              wps, (ull)entry, (ull)one);
        for (uint64_t c : rows)
            for (uint64_t s : singles)
                for (uint64_t e : entries) {
                    CHECK(digest_tile_fits(std::min<uint64_t>(c, DIGEST_ROWS_MAX), c, s, e), "%llu %llu %llu", (ull)c, (ull)s, (ull)e);
                    const uint64_t bound = digest_lane_sum_bound(c, s, e);
                    CHECK(bound < (1ull << 32), "bound %llu at %llu rows %llu singletons %llu entries", (ull)bound, (ull)c, (ull)s, (ull)e);
                    const uint64_t words = s ? (s + 3) / 4 + 1 : 0;  // a range that begins and ends inside a word
                    const uint64_t hist = s * one, range = ((words + 63) / 64) * 4 * one;
                    const uint64_t lane = c * row + std::max(hist, range) + ((e + 63) / 64) * entry;
                    CHECK(lane <= bound, "wps %u: lane %llu > bound %llu at %llu rows %llu singletons %llu entries", wps, (ull)lane, (ull)bound,
                          (ull)c, (ull)s, (ull)e);
                    worst_seen = std::max(worst_seen, lane);
                    ++sizes;
                }
    }
    CHECK(!digest_tile_fits(DIGEST_ROWS_MAX + 1, DIGEST_ROWS_MAX + 1, 0, 0) && !digest_tile_fits(1, DIGEST_COMMON_MAX + 1, 0, 0) &&
              !digest_tile_fits(0, 0, DIGEST_SINGLES_MAX + 1, 0) && !digest_tile_fits(0, 0, 0, WAVE_RARE_WORDS_MAX + 1),
          "one above a cap fits");
    CHECK(digest_tile_fits(DIGEST_ROWS_MAX, DIGEST_COMMON_MAX, DIGEST_SINGLES_MAX, WAVE_RARE_WORDS_MAX), "the caps do not fit");
    // above the cap the bound itself passes 2^32: the cap is what keeps the sums right
    CHECK(digest_lane_sum_bound(2 * DIGEST_COMMON_MAX, 0, 0) >= (1ull << 32), "the row cap is not what binds");
    printf("bound ok sizes=%llu worst=%llu\n", (ull)sizes, (ull)worst_seen);
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
    uint64_t s = seed;
    for (uint64_t it = 0; it < count; ++it) {
        const uint32_t wps = 1 + (uint32_t)(rnd(s) % 16);
        const size_t nt = (size_t)(rnd(s) % 40);
        const bool packed = rnd(s) % 4 != 0;
        std::vector<ScanTile> tiles(nt);
        std::vector<SingleRange> singles(packed ? nt : 0);
        std::vector<uint32_t> reps(nt);
        uint64_t site = rnd(s) % 200, rare = rnd(s) % 50, single = rnd(s) % 9, plain = 0;
        bool all_fit = true;
        for (size_t k = 0; k < nt; ++k) {
            const uint64_t rows = rnd(s) % 5 == 0 ? 0 : rnd(s) % 700, ne = rnd(s) % 3 == 0 ? 0 : rnd(s) % 300;
            // singleton ranges around the histogram's length, 8 wps singletons' worth of words, and anywhere
            const uint64_t ns = rnd(s) % 4 == 0 ? 0 : rnd(s) % 2 ? 32ull * wps - 8 + rnd(s) % 16 : rnd(s) % 70000;
            tiles[k] = {site, site + rows, rare, rare + ne};
            site += rows + rnd(s) % 3; rare += ne;
            if (packed) { singles[k] = {single, single + ns}; single += ns; }
            const SingleRange sr = packed ? singles[k] : SingleRange{0, 0};
            const uint64_t cand = digest_candidates(tiles[k], UniqRange{0, 0});
            CHECK(cand == rows, "candidates of a tile without a range");
            all_fit = all_fit && digest_tile_fits(tiles[k], UniqRange{0, 0}, sr);
            reps[k] = (uint32_t)(rows ? 1 + rnd(s) % std::min<uint64_t>(rows, DIGEST_ROWS_MAX) : 0);
            plain += tile_bytes_streamed(tiles[k], wps) + single_bytes_streamed(sr);
        }
        DigestLayout L;
        digest_layout(tiles, singles, reps.data(), wps, L);
        CHECK(L.descs.size() == nt, "descs");
        uint64_t next_row = 0, n_rows = 0, hist = 0, read = 0, dbytes = 0;
        for (size_t k = 0; k < nt; ++k) {
            const DigestDesc &d = L.descs[k];
            const SingleRange sr = packed ? singles[k] : SingleRange{0, 0};
            CHECK(d.row_off == next_row && d.row_off % DIGEST_ROW_GRAIN == 0, "tile %zu: row_off %llu, expected %llu", k, (ull)d.row_off, (ull)next_row);
            CHECK((d.row_off * 4 * wps) % 16 == 0 && (d.row_off * 2) % 8 == 0, "tile %zu: alignment", k);
            CHECK(d.n_rows == reps[k], "tile %zu: n_rows", k);
            const uint64_t padded = digest_rows_padded(d.n_rows);
            CHECK(padded >= d.n_rows && padded < d.n_rows + DIGEST_ROW_GRAIN && padded % DIGEST_ROW_GRAIN == 0, "padding");
            // the last dword a lane of the kernel reads of this tile lies in the tile's own rows
            if (d.n_rows) {
                const uint32_t G = (wps + 3) / 4, r = wps - 4 * (G - 1);
                const uint64_t last = (uint64_t)(G - 1) * padded * 4 + (uint64_t)(d.n_rows - 1) * r + r - 1;
                CHECK(last < padded * wps, "tile %zu: a row ends past the tile", k);
                if (G > 1) CHECK(((uint64_t)(G - 2) * padded + d.n_rows - 1) * 4 + 3 < (uint64_t)(G - 1) * padded * 4, "a granule runs into the next section");
            }
            next_row += padded;
            n_rows += d.n_rows;
            const bool want_hist = sr.end > sr.begin && single_bytes_streamed(sr) >= 64ull * wps;
            CHECK((d.hist != 0) == want_hist, "tile %zu: histogram", k);
            uint64_t tile_read = padded * (4ull * wps + 2) + (tiles[k].rare_end - tiles[k].rare_begin) * 8;
            if (d.hist) {
                CHECK(d.hist == ++hist && d.single_begin == d.single_end, "tile %zu: histogram index", k);
                tile_read += 64ull * wps;
                CHECK(64ull * wps <= single_bytes_streamed(sr), "a histogram longer than the range it replaces");
            } else {
                CHECK(d.single_begin == sr.begin && d.single_end == (sr.end > sr.begin ? sr.end : sr.begin), "tile %zu: kept range", k);
                tile_read += single_bytes_streamed(sr);
            }
            CHECK(d.rare_begin == tiles[k].rare_begin && d.rare_end == tiles[k].rare_end, "tile %zu: entries", k);
            read += tile_read;
            dbytes += padded * (4ull * wps + 2) + (d.hist ? 64ull * wps : 0);
        }
        CHECK(L.n_rows == n_rows && L.rows_padded == next_row && L.n_hist_tiles == hist, "totals");
        CHECK(L.digest_bytes() == dbytes, "digest_bytes %llu, the tiles add up to %llu", (ull)L.digest_bytes(), (ull)dbytes);
        CHECK(L.bytes_streamed() == read && L.bytes_streamed() == L.rows_streamed() + L.rare_streamed(), "bytes_streamed %llu, the tiles read %llu",
              (ull)L.bytes_streamed(), (ull)read);
        // the three sections of the allocation do not overlap and keep their alignment
        CHECK(L.weight_offset() == L.row_bytes && L.weight_offset() % 16 == 0, "weights");
        CHECK(L.hist_offset() >= L.weight_offset() + L.weight_bytes && L.hist_offset() % 16 == 0 && L.hist_offset() < L.weight_offset() + L.weight_bytes + 16, "histograms");
        CHECK(L.alloc_bytes() == L.hist_offset() + L.hist_bytes, "allocation");
        // the rule and the overrides
        const bool wave = rnd(s) % 4 != 0, reusable = rnd(s) % 3 != 0;
        const uint64_t with = L.bytes_streamed();
        for (uint64_t without : {plain, with, with + 1, with ? with - 1 : 0}) {
            const bool rule = digest_choice(-1, reusable, wave, all_fit, with, without);
            CHECK(rule == (reusable && wave && all_fit && with <= without), "the rule");
            CHECK(!rule || with <= without, "the rule takes a plan that reads more with the digest");
            CHECK(!digest_choice(0, reusable, wave, all_fit, with, without), "override 0");
            CHECK(digest_choice(1, reusable, wave, all_fit, with, without) == (wave && all_fit), "override 1");
            CHECK(digest_wanted(-1, reusable, wave, all_fit) == (reusable && wave && all_fit) && digest_wanted(1, reusable, wave, all_fit) == (wave && all_fit) &&
                      !digest_wanted(0, reusable, wave, all_fit), "wanted");
        }
    }
    printf("random ok n=%llu\n", (ull)count);
    return 0;
}

int main(int argc, char **argv) {
    auto num = [&](int i) { return strtoull(argv[i], nullptr, 10); };
    if (argc == 2 && !strcmp(argv[1], "bound")) return run_bound();
    if (argc == 4 && !strcmp(argv[1], "random")) return run_random(num(2), num(3));
    if (argc == 6 && !strcmp(argv[1], "fits")) {
        printf("fits=%d\n", (int)digest_tile_fits(num(2), num(3), num(4), num(5)));
        return 0;
    }
    if (argc == 6 && !strcmp(argv[1], "candidates")) {
        printf("candidates=%llu\n", (ull)digest_candidates(ScanTile{num(2), num(3), 0, 0}, UniqRange{num(4), num(5)}));
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "hist")) {
        printf("hist=%d\n", (int)digest_takes_hist(SingleRange{num(2), num(3)}, (uint32_t)num(4)));
        return 0;
    }
    if (argc == 8 && !strcmp(argv[1], "choice")) {
        printf("digest=%d\n", (int)digest_choice(atoi(argv[2]), num(3) != 0, num(4) != 0, num(5) != 0, num(6), num(7)));
        return 0;
    }
    fprintf(stderr, "usage: tile_digest bound | random SEED N | fits ... | candidates ... | hist ... | choice ...\n");
    return 2;
}
