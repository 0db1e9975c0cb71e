// ibd_chain.cc — stand-alone driver for csrc/ibd_chain.h (no GPU, built with ASan + UBSan by tests/test_ibd_chain_host.py).
//   ibd_chain <seed> <rounds>
// Per round: a random map (or none), a random ascending tract list and random thresholds.  The list goes through
// ibd_chain_batch in random batch sizes of 1..130 (a batch above 64 is handed over in wave-sized pieces, as the kernel does) and
// the segments are compared with a direct evaluation of the definition.  ibd_map_eval is checked against 128-bit arithmetic at
// the breakpoints, next to them and outside the map.  Prints "ok <rounds>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "ibd_chain.h"

using namespace impop;

struct Seg {
    uint64_t begin, end, len;
    uint32_t n, sites;
    bool operator==(const Seg &o) const { return begin == o.begin && end == o.end && len == o.len && n == o.n && sites == o.sites; }
};

static uint64_t eval128(const std::vector<uint64_t> &pos, const std::vector<uint64_t> &g, uint64_t x) {
    if (pos.empty()) return x;
    if (x <= pos.front()) return g.front();
    if (x >= pos.back()) return g.back();
    size_t k = 0;
    while (!(pos[k] <= x && x < pos[k + 1])) ++k;
    const unsigned __int128 num = (unsigned __int128)(x - pos[k]) * (unsigned __int128)(g[k + 1] - g[k]);
    return g[k] + (uint64_t)(num / (unsigned __int128)(pos[k + 1] - pos[k]));
}

#define CHECK(c, ...)                     \
    do {                                  \
        if (!(c)) {                       \
            fprintf(stderr, __VA_ARGS__); \
            fprintf(stderr, "\n");        \
            return 1;                     \
        }                                 \
    } while (0)

int main(int argc, char **argv) {
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int rounds = argc > 2 ? atoi(argv[2]) : 100;
    std::mt19937_64 rng(seed);
    auto U = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
    for (int r = 0; r < rounds; ++r) {
        // the map: steps up to just below 2^32 in some rounds, zero-rate intervals, breakpoints outside the tracts' span
        std::vector<uint64_t> pos, g;
        const bool big = r % 7 == 0;
        const uint64_t coord0 = big ? U(0, 1ull << 40) : U(0, 50);
        if (r % 3 != 0) {
            const uint32_t n = (uint32_t)U(2, 40);
            uint64_t p = coord0 + U(0, 30) - std::min<uint64_t>(coord0, U(0, 30)), gg = U(0, 1000);
            for (uint32_t k = 0; k < n; ++k) {
                pos.push_back(p);
                g.push_back(gg);
                p += big ? U(1, (1ull << 32) - 1) : U(1, 60);
                gg += U(0, 3) == 0 ? 0 : (big ? U(0, (1ull << 32) - 1) : U(0, 90));
            }
            CHECK(ibd_map_check(pos.data(), g.data(), n) == 0, "round %d: a good map was refused", r);
        }
        IbdMap map;
        map.pos = pos.data();
        map.g = g.data();
        map.n = (uint32_t)pos.size();
        for (size_t k = 0; k < pos.size(); ++k)
            for (int d = -1; d <= 1; ++d) {
                if (d < 0 && pos[k] == 0) continue;
                const uint64_t x = pos[k] + d;
                CHECK(ibd_map_eval(map, x) == eval128(pos, g, x), "round %d: G(%llu) differs from 128-bit arithmetic", r, (unsigned long long)x);
            }
        for (int q = 0; q < 40; ++q) {
            const uint64_t x = pos.empty() ? U(0, 1000) : U(pos.front() > 5 ? pos.front() - 5 : 0, pos.back() + 5);
            CHECK(ibd_map_eval(map, x) == eval128(pos, g, x), "round %d: G(%llu) differs from 128-bit arithmetic", r, (unsigned long long)x);
        }

        // tracts: ascending, at least one coordinate between two of them
        const uint32_t nt = (uint32_t)(big ? U(0, 10) : U(0, 400));  // big: the sums stay below 2^32
        const uint64_t scale = big ? (1ull << 22) : 1;
        std::vector<uint64_t> s(nt), t(nt);
        uint64_t x = coord0;
        for (uint32_t i = 0; i < nt; ++i) {
            x += (i ? 1 : 0) + (U(0, 2) ? 0 : U(0, 6) * scale);
            s[i] = x;
            x += U(1, U(0, 4) ? 12 : 80) * scale;
            t[i] = x;
        }
        CHECK(nt == 0 || t[nt - 1] - s[0] < (1ull << 32), "round %d: the driver's own range is too long", r);
        IbdRule rule;
        rule.min_sites = (uint32_t)(U(1, 9) * scale);
        rule.min_extend = U(0, 30) * (map.n ? 3 : 1) * scale;
        rule.min_seed = rule.min_extend + U(0, 60) * scale;
        rule.min_output = U(0, 200) * scale;
        rule.max_gap = U(0, 3) ? U(0, 8) * scale : (U(0, 1) ? 0 : ~0ull);

        // the definition, directly
        std::vector<Seg> want;
        uint32_t want_cand = 0;
        {
            bool open = false, seed_in = false;
            Seg cur{};
            uint64_t prev_end = 0;
            auto close = [&] {
                if (open && seed_in && cur.len >= rule.min_output) want.push_back(cur);
            };
            for (uint32_t i = 0; i < nt; ++i) {
                const uint64_t len = eval128(pos, g, t[i]) - eval128(pos, g, s[i]);
                if (t[i] - s[i] < rule.min_sites || len < rule.min_extend) continue;
                ++want_cand;
                if (!open || s[i] - prev_end > rule.max_gap) {
                    close();
                    cur = Seg{s[i], t[i], 0, 0, 0};
                    open = true;
                    seed_in = false;
                }
                cur.end = t[i];
                cur.len = eval128(pos, g, cur.end) - eval128(pos, g, cur.begin);
                cur.n += 1;
                cur.sites += (uint32_t)(t[i] - s[i]);
                seed_in = seed_in || len >= rule.min_seed;
                prev_end = t[i];
            }
            close();
        }

        // the batched step
        std::vector<Seg> got;
        uint32_t got_cand = 0;
        auto emit = [&](const IbdChain &c) { got.push_back(Seg{c.begin, c.end, c.gend - c.gbegin, c.n, c.sites}); };
        IbdChain c;
        for (uint32_t i = 0; i < nt;) {
            const uint32_t batch = (uint32_t)std::min<uint64_t>(U(1, 130), nt - i);
            for (uint32_t j = 0; j < batch; j += 64)
                ibd_chain_batch(c, s.data() + i + j, t.data() + i + j, std::min(64u, batch - j), map, rule, &got_cand, emit);
            i += batch;
        }
        ibd_chain_finish(c, rule, emit);
        CHECK(got_cand == want_cand, "round %d: %u candidates, the definition has %u", r, got_cand, want_cand);
        CHECK(got.size() == want.size(), "round %d: %zu segments, the definition has %zu", r, got.size(), want.size());
        for (size_t i = 0; i < got.size(); ++i)
            CHECK(got[i] == want[i], "round %d: segment %zu is [%llu,%llu) len %llu n %u sites %u, the definition has [%llu,%llu) len %llu n %u sites %u",
                  r, i, (unsigned long long)got[i].begin, (unsigned long long)got[i].end, (unsigned long long)got[i].len, got[i].n, got[i].sites,
                  (unsigned long long)want[i].begin, (unsigned long long)want[i].end, (unsigned long long)want[i].len, want[i].n, want[i].sites);
    }
    // refusals of the map check
    {
        const uint64_t p1[3] = {1, 5, 5}, g1[3] = {0, 1, 2}, p2[2] = {0, 1ull << 32}, g2[2] = {0, 1}, p3[2] = {0, 9}, g3[2] = {5, 4};
        CHECK(ibd_map_check(p1, g1, 3) == 2 && ibd_map_check(p2, g2, 2) == 1 && ibd_map_check(p3, g3, 2) == 1, "a bad map was accepted");
    }
    printf("ok %d\n", rounds);
    return 0;
}
