// dip_runs.cc — host check of csrc/dip_runs.h, the run-length summary of impop_diploid_scan (plain C++, no HIP, no GPU; built
// with -fsanitize=address,undefined by tests/test_dip_runs_host.py).
//
//   dip_runs <seed> <cases>
//
// Per case: a random window [b, e) in 64-bit coordinates, a random set of heterozygous sites in it (empty, sparse, dense, with
// sites at b and at e - 1), cut into random "tiles", every tile cut further at random "wave" boundaries.  Every piece is folded
// site by site (dip_append_site), the pieces of a tile are joined in order (dip_combine), the tiles are joined in order, the
// window's edges close the result (dip_close).  The outcome must equal a direct scan of the definition in include/impop_hip.h for
// min_run in {1, 2, 7, 64, 65}; it must not depend on where the cuts are (a second, different cutting and the uncut fold give the
// same summary: associativity), empty pieces are neutral, and run_sum + het == e - b.  Prints "ok <cases>" or the first mismatch.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "dip_runs.h"

using impop::DipSummary;

static uint64_t rng_state;
static uint64_t rnd() {  // splitmix64
    uint64_t x = (rng_state += 0x9E3779B97F4A7C15ull);
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}
static uint64_t below(uint64_t n) { return n ? rnd() % n : 0; }

struct Direct {
    uint32_t het, longest, roh_runs, roh_sites;
};

// the definition, spelled out: runs p_1 - b, p_{j+1} - p_j - 1, e - 1 - p_k; none heterozygous: one run of e - b
static Direct direct(const std::vector<uint64_t> &p, uint64_t b, uint64_t e, uint32_t min_run) {
    std::vector<uint64_t> runs;
    if (p.empty()) {
        runs.push_back(e - b);
    } else {
        runs.push_back(p.front() - b);
        for (size_t j = 0; j + 1 < p.size(); ++j) runs.push_back(p[j + 1] - p[j] - 1);
        runs.push_back(e - 1 - p.back());
    }
    Direct d{(uint32_t)p.size(), 0, 0, 0};
    for (uint64_t r : runs) {
        if (r == 0) continue;
        d.longest = std::max<uint32_t>(d.longest, (uint32_t)r);
        if (r >= min_run) {
            d.roh_runs += 1;
            d.roh_sites += (uint32_t)r;
        }
    }
    return d;
}

// sorted cut points in [b, e], b and e included
static std::vector<uint64_t> cuts(uint64_t b, uint64_t e, uint32_t n) {
    std::vector<uint64_t> c{b, e};
    for (uint32_t k = 0; k < n; ++k) c.push_back(b + below(e - b + 1));
    std::sort(c.begin(), c.end());
    return c;
}

// the sites of p inside [lo, hi), folded one by one; hom sites are handed out so that every piece gets some
static DipSummary fold_piece(const std::vector<uint64_t> &p, uint64_t lo, uint64_t hi, uint32_t min_run, uint32_t hom) {
    DipSummary s = impop::dip_empty();
    s.hom_alt = hom;
    for (auto it = std::lower_bound(p.begin(), p.end(), lo); it != p.end() && *it < hi; ++it) impop::dip_append_site(s, *it, min_run);
    return s;
}

static DipSummary fold_cut(const std::vector<uint64_t> &p, uint64_t b, uint64_t e, uint32_t min_run, uint32_t n_tiles, uint32_t n_waves,
                           uint32_t *hom_total) {
    const std::vector<uint64_t> tc = cuts(b, e, n_tiles);
    DipSummary win = impop::dip_empty();
    for (size_t t = 0; t + 1 < tc.size(); ++t) {
        const std::vector<uint64_t> wc = cuts(tc[t], tc[t + 1], n_waves);
        DipSummary tile = impop::dip_empty();
        for (size_t w = 0; w + 1 < wc.size(); ++w) {
            const uint32_t hom = (uint32_t)below(5);
            *hom_total += hom;
            tile = impop::dip_combine(tile, fold_piece(p, wc[w], wc[w + 1], min_run, hom), min_run);
        }
        win = impop::dip_combine(win, tile, min_run);
    }
    return win;
}

static bool same(const DipSummary &a, const DipSummary &b) {
    return a.het == b.het && (a.het == 0 || (a.first == b.first && a.last == b.last)) && a.longest == b.longest && a.roh_runs == b.roh_runs &&
           a.roh_sites == b.roh_sites && a.run_sum == b.run_sum;
}

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: dip_runs <seed> <cases>\n");
        return 2;
    }
    rng_state = strtoull(argv[1], nullptr, 10);
    const uint64_t n_cases = strtoull(argv[2], nullptr, 10);
    static const uint32_t MIN_RUNS[5] = {1, 2, 7, 64, 65};
    static_assert(sizeof(DipSummary) == 40, "the device stores 40-byte summaries");
    for (uint64_t k = 0; k < n_cases; ++k) {
        // coordinates anywhere in 64 bits (a compacted matrix hands in original positions), windows of 1 .. 3000 sites and a few long ones
        const uint64_t b = (k % 3 == 0) ? below(1000) : (rnd() >> (1 + below(40)));
        const uint64_t W = (k % 17 == 0) ? 1 + below(0xFFFFFFFEull) : 1 + below(k % 5 == 0 ? 130 : 3000);
        const uint64_t e = b + W;
        std::vector<uint64_t> p;
        const uint32_t style = (uint32_t)below(5);  // 0: none, 1: sparse, 2: dense, 3: both edges + sparse, 4: every site of a short stretch
        const uint64_t span = std::min<uint64_t>(W, 3000);
        if (style == 1 || style == 3)
            for (uint32_t i = 0, m = (uint32_t)below(12); i < m; ++i) p.push_back(b + below(W));
        if (style == 2)
            for (uint64_t s = 0; s < span; ++s)
                if (below(3) == 0) p.push_back(b + s);
        if (style == 3) {
            p.push_back(b);
            p.push_back(e - 1);
        }
        if (style == 4)
            for (uint64_t s = below(span), end = std::min<uint64_t>(span, s + 1 + below(70)); s < end; ++s) p.push_back(b + s);
        std::sort(p.begin(), p.end());
        p.erase(std::unique(p.begin(), p.end()), p.end());
        for (uint32_t min_run : MIN_RUNS) {
            const Direct want = direct(p, b, e, min_run);
            uint32_t hom1 = 0, hom2 = 0, hom0 = 0;
            const DipSummary s1 = fold_cut(p, b, e, min_run, (uint32_t)below(9), (uint32_t)below(4), &hom1);
            const DipSummary s2 = fold_cut(p, b, e, min_run, (uint32_t)below(40), 3, &hom2);
            const DipSummary s0 = fold_cut(p, b, e, min_run, 0, 0, &hom0);  // uncut
            if (!same(s1, s0) || !same(s2, s0) || s1.hom_alt != hom1 || s2.hom_alt != hom2 || s0.hom_alt != hom0) {
                printf("case %llu min_run %u: the summary depends on the cuts\n", (unsigned long long)k, min_run);
                return 1;
            }
            const DipSummary c = impop::dip_close(s1, b, e, min_run);
            if (c.het != want.het || c.longest != want.longest || c.roh_runs != want.roh_runs || c.roh_sites != want.roh_sites ||
                (uint64_t)c.run_sum + c.het != W) {
                printf("case %llu min_run %u: got het %u longest %u runs %u sites %u run_sum %u, want %u %u %u %u (W %llu)\n",
                       (unsigned long long)k, min_run, c.het, c.longest, c.roh_runs, c.roh_sites, c.run_sum, want.het, want.longest,
                       want.roh_runs, want.roh_sites, (unsigned long long)W);
                return 1;
            }
        }
    }
    printf("ok %llu\n", (unsigned long long)n_cases);
    return 0;
}
