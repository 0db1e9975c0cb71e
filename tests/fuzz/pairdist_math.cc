// Stand-alone driver for csrc/pairdist_math.h (no HIP): random small distance matrices over random panels are cut into random
// tiles, the tiles folded with pd_acc_add / pd_nn_add and merged in random order with pd_acc_merge / pd_nn_merge, and the records'
// fields, the nearest-neighbour counts, the bits of snn and gmin and the sum_h2 admission rule at its boundary must equal a direct
// scan of the definitions.  Build with -fsanitize=address,undefined.   usage: pairdist_math <seed> <iterations>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <vector>

#include "pairdist_math.h"

using namespace impop;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            printf("FAILED %s (line %d, iteration %d)\n", #cond, __LINE__, it); \
            return 1;                                                        \
        }                                                                    \
    } while (0)

static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }

int main(int argc, char **argv) {
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int iters = argc > 2 ? atoi(argv[2]) : 1000;
    std::mt19937_64 rng(seed);
    auto below = [&](uint32_t n) { return (uint32_t)(rng() % n); };
    int it = 0;
    // the admission rule: W^2 P <= 2^64 - 1, checked against 128-bit arithmetic at and around the boundary
    for (it = 0; it < iters; ++it) {
        const uint64_t P = 1 + rng() % (1ull << (1 + below(23)));
        uint64_t lo = 0, hi = 0x100000000ull;  // the largest W with W^2 P <= max
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo + 1) / 2;
            if ((unsigned __int128)mid * mid * P <= (unsigned __int128)0xFFFFFFFFFFFFFFFFull) lo = mid; else hi = mid - 1;
        }
        CHECK(pd_sum_h2_admitted(lo, P) && !pd_sum_h2_admitted(lo + 1, P));
        const uint64_t W = rng() >> below(64);
        CHECK(pd_sum_h2_admitted(W, P) == ((unsigned __int128)W * W * P <= (unsigned __int128)0xFFFFFFFFFFFFFFFFull || W == 0));
    }
    CHECK(pd_sum_h2_admitted(0, 12345) && pd_sum_h2_admitted(1ull << 31, 0) && pd_sum_h2_admitted(0xFFFFFFFFull, 1));
    CHECK(!pd_sum_h2_admitted(0x100000000ull, 1) && pd_sum_h2_admitted(200000063ull, 780) == false && pd_sum_h2_admitted(100000063ull, 780));

    for (it = 0; it < iters; ++it) {
        const uint32_t K = 1 + below(4), n_hap = K + below(20);
        // panels: every haplotype in one of K panels or in none; none empty
        std::vector<uint32_t> cls(n_hap);
        for (uint32_t i = 0; i < n_hap; ++i) cls[i] = i < K ? i : below(K + 1);
        std::shuffle(cls.begin(), cls.end(), rng);
        std::vector<uint32_t> hap_of, off(K + 1, 0);
        for (uint32_t k = 0; k < K; ++k) {
            off[k] = (uint32_t)hap_of.size();
            for (uint32_t i = 0; i < n_hap; ++i) if (cls[i] == k) hap_of.push_back(i);
        }
        off[K] = (uint32_t)hap_of.size();
        const uint32_t M = off[K];
        // distances over positions, few distinct values (ties), now and then the largest ones
        const uint32_t top = below(8) == 0 ? 0x80000000u : 1 + below(6);
        std::vector<uint32_t> H((size_t)M * M, 0);
        for (uint32_t p = 0; p < M; ++p)
            for (uint32_t q = p + 1; q < M; ++q) H[(size_t)p * M + q] = H[(size_t)q * M + p] = top > 6 ? top - below(3) : below(top + 1);
        auto panel_of = [&](uint32_t p) { uint32_t c = 0; while (off[c + 1] <= p) ++c; return c; };
        const uint32_t NP = K * (K - 1) / 2, R = K + NP;
        auto rec_of = [&](uint32_t p, uint32_t q) {  // p < q
            const uint32_t a = panel_of(p), b = panel_of(q);
            return a == b ? a : K + pd_pair_index(K, a, b);
        };
        // ---- tiles: the ordered entries (p, q), p != q, dealt to random tiles; a tile folds its entries, tiles merge in random order
        struct Entry { uint32_t p, q; };
        std::vector<Entry> entries;
        for (uint32_t p = 0; p < M; ++p) for (uint32_t q = 0; q < M; ++q) if (p != q) entries.push_back({p, q});
        std::shuffle(entries.begin(), entries.end(), rng);
        const uint32_t n_tiles = 1 + below(7);
        std::vector<std::vector<DistAcc>> acc(n_tiles, std::vector<DistAcc>(R, pd_acc_empty()));
        std::vector<std::vector<DistNN>> nn(n_tiles, std::vector<DistNN>((size_t)M * K, pd_nn_empty()));
        for (const Entry &e : entries) {
            const uint32_t t = below(n_tiles), h = H[(size_t)e.p * M + e.q];
            pd_nn_add(nn[t][(size_t)e.p * K + panel_of(e.q)], h);
            if (e.p < e.q) pd_acc_add(acc[t][rec_of(e.p, e.q)], h, e.p, e.q);
        }
        std::vector<uint32_t> order(n_tiles);
        for (uint32_t t = 0; t < n_tiles; ++t) order[t] = t;
        std::shuffle(order.begin(), order.end(), rng);
        std::vector<DistAcc> A(R, pd_acc_empty());
        std::vector<DistNN> N((size_t)M * K, pd_nn_empty());
        for (uint32_t t : order) {
            for (uint32_t r = 0; r < R; ++r) A[r] = below(2) ? pd_acc_merge(A[r], acc[t][r]) : pd_acc_merge(acc[t][r], A[r]);
            for (size_t i = 0; i < N.size(); ++i) N[i] = below(2) ? pd_nn_merge(N[i], nn[t][i]) : pd_nn_merge(nn[t][i], N[i]);
        }
        // ---- the direct scan, in haplotype terms
        for (uint32_t r = 0; r < R; ++r) {
            uint32_t a = r, b = r;
            if (r >= K) { uint32_t rest = r - K; a = 0; while (rest >= K - 1 - a) { rest -= K - 1 - a; ++a; } b = a + 1 + rest; }
            CHECK(r < K || pd_pair_index(K, a, b) == r - K);
            uint64_t n_pairs = 0, sum_h = 0, sum_h2 = 0, n_zero = 0;
            uint32_t min_h = 0, max_h = 0, mi = PAIRDIST_NONE, mj = PAIRDIST_NONE, xi = PAIRDIST_NONE, xj = PAIRDIST_NONE;
            for (uint32_t p = off[a]; p < off[a + 1]; ++p)          // ascending i, then ascending j: the first of the ties wins
                for (uint32_t q = (a == b ? p + 1 : off[b]); q < off[b + 1]; ++q) {
                    const uint32_t h = H[(size_t)p * M + q];
                    if (n_pairs == 0 || h < min_h) { min_h = h; mi = hap_of[p]; mj = hap_of[q]; }
                    if (n_pairs == 0 || h > max_h) { max_h = h; xi = hap_of[p]; xj = hap_of[q]; }
                    ++n_pairs; sum_h += h; sum_h2 += (uint64_t)h * h; n_zero += h == 0;
                }
            const DistFields f = pd_fields(A[r], n_pairs, hap_of.data());
            CHECK(f.sum_h == sum_h && f.sum_h2 == sum_h2 && f.n_zero == n_zero && f.min_h == min_h && f.max_h == max_h);
            CHECK(f.min_i == mi && f.min_j == mj && f.max_i == xi && f.max_j == xj);
            if (a != b) CHECK(mi == PAIRDIST_NONE || (cls[mi] == a && cls[mj] == b));
            if (r < K) continue;
            // nearest neighbours of the pair (a, b): members in ascending haplotype index
            std::vector<uint32_t> both;
            for (uint32_t p = off[a]; p < off[a + 1]; ++p) both.push_back(p);
            for (uint32_t p = off[b]; p < off[b + 1]; ++p) both.push_back(p);
            std::sort(both.begin(), both.end(), [&](uint32_t x, uint32_t y) { return hap_of[x] < hap_of[y]; });
            double direct = 0.0, folded = 0.0;
            uint32_t cnt[4] = {0, 0, 0, 0}, got[4] = {0, 0, 0, 0};
            for (uint32_t p : both) {
                uint32_t d = PAIRDIST_NONE, tied = 0, same = 0;
                for (uint32_t q : both) if (q != p) d = std::min(d, H[(size_t)p * M + q]);
                for (uint32_t q : both) if (q != p && H[(size_t)p * M + q] == d) { ++tied; same += panel_of(q) == panel_of(p); }
                const bool in_a = panel_of(p) == a;
                direct += (double)same / (double)tied;
                cnt[in_a ? 0 : 1] += same == tied; cnt[in_a ? 2 : 3] += same == 0;
                uint32_t t2, s2;
                pd_nn_pair(N[(size_t)p * K + (in_a ? a : b)], N[(size_t)p * K + (in_a ? b : a)], &t2, &s2);
                CHECK(t2 == tied && s2 == same);
                folded += pd_snn_term(s2, t2);
                got[in_a ? 0 : 1] += s2 == t2; got[in_a ? 2 : 3] += s2 == 0;
            }
            CHECK(memcmp(cnt, got, sizeof cnt) == 0);
            CHECK(same_bits(pd_snn_finish(folded, (uint32_t)both.size()), direct / (double)both.size()));
            const double g = pd_gmin(f.min_h, f.sum_h, n_pairs);
            if (sum_h == 0) CHECK(g != g && same_bits(g, __builtin_nan("")));
            else CHECK(same_bits(g, (double)min_h / ((double)sum_h / (double)n_pairs)));
        }
        // bins: the last one collects the overflow
        const uint32_t bins = 1 + below(9), width = 1 + below(5), h = below(60);
        CHECK(pd_bin(h, width, bins) == std::min(h / width, bins - 1) && pd_bin(0x80000000u, 1, 1024) == 1023);
    }
    printf("ok %d\n", iters);
    return 0;
}
