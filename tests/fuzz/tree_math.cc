// Stand-alone driver for csrc/tree_math.h (no HIP): tree_solve_serial — the cached-neighbour scheme of the kernel — against a
// brute-force global search over all live pairs per step, written here with unsigned __int128 and nothing shared with the header,
// on random small integer matrices with many ties, the three linkages and random panels; the value comparison against
// unsigned __int128 at extreme operands (numerators up to 2^49, denominators up to 2^18); the 64 x 64 -> 128 multiply.
// Build with -fsanitize=address,undefined.   usage: tree_math <seed> <iterations>
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "tree_math.h"

using namespace impop;
typedef unsigned __int128 u128;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            printf("FAILED %s (line %d, iteration %d)\n", #cond, __LINE__, it); \
            return 1;                                                        \
        }                                                                    \
    } while (0)

struct BruteResult {
    std::vector<TreeMerge> merges;
    std::vector<TreePanel> panels;
    uint32_t n_zero = 0, n_tied = 0;
};
// the definition: clusters as member lists, every value recomputed from H, every pair of live clusters compared
static BruteResult brute(const std::vector<uint64_t> &H, uint32_t m, uint32_t linkage, const std::vector<uint8_t> &cls, uint32_t K) {
    BruteResult R;
    std::vector<std::vector<uint32_t>> members(m);
    for (uint32_t i = 0; i < m; ++i) members[i] = {i};
    std::vector<uint32_t> psize(K, 0);
    for (uint32_t i = 0; i < m; ++i)
        if (cls[i] < K) ++psize[cls[i]];
    for (uint32_t p = 0; p < K; ++p) R.panels.push_back(TreePanel{psize[p], 1u, psize[p] == 1 ? 1u : 0u, 0xFFFFFFFFu});
    for (uint32_t step = 0; step + 1 < m; ++step) {
        bool have = false;
        uint64_t bn = 0, bd = 1;
        uint32_t ba = 0, bb = 0, at_min = 0;
        for (uint32_t a = 0; a < m; ++a) {
            if (members[a].empty()) continue;
            for (uint32_t b = a + 1; b < m; ++b) {
                if (members[b].empty()) continue;
                uint64_t mn = ~0ull, mx = 0, sum = 0;
                for (uint32_t i : members[a])
                    for (uint32_t j : members[b]) {
                        const uint64_t h = H[(size_t)i * m + j];
                        mn = h < mn ? h : mn; mx = h > mx ? h : mx; sum += h;
                    }
                const uint64_t n = linkage == 0 ? mn : linkage == 1 ? mx : sum;
                const uint64_t d = linkage == 2 ? (uint64_t)members[a].size() * members[b].size() : 1;
                const u128 l = (u128)n * bd, r = (u128)bn * d;
                if (!have || l < r) { have = true; bn = n; bd = d; ba = a; bb = b; at_min = 1; }  // (a, b) ascend: the first wins ties
                else if (l == r) ++at_min;
            }
        }
        const uint32_t sa = (uint32_t)members[ba].size(), sb = (uint32_t)members[bb].size();
        R.merges.push_back(TreeMerge{ba, bb, sa, sb, bn});
        R.n_zero += bn == 0;
        R.n_tied += at_min >= 2;
        members[ba].insert(members[ba].end(), members[bb].begin(), members[bb].end());
        members[bb].clear();
        for (uint32_t p = 0; p < K; ++p) {
            uint32_t inside = 0;
            for (uint32_t i : members[ba]) inside += cls[i] == p;
            if (inside == sa + sb && sa + sb > R.panels[p].largest_clade) R.panels[p].largest_clade = sa + sb;
            if (R.panels[p].mrca_size == 0 && inside == R.panels[p].n_members) { R.panels[p].mrca_size = sa + sb; R.panels[p].mrca_merge = step; }
        }
    }
    return R;
}

int main(int argc, char **argv) {
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int iters = argc > 2 ? atoi(argv[2]) : 100;
    std::mt19937_64 rng(seed);
    auto below = [&](uint64_t n) { return (uint64_t)(rng() % n); };
    int it = -1;

    // the multiply and the comparison against unsigned __int128
    for (int t = 0; t < 200000; ++t) {
        const uint64_t x = rng() >> below(64), y = rng() >> below(64);
        const TreeU128 p = tree_mul_64x64(x, y);
        const u128 want = (u128)x * y;
        CHECK(p.hi == (uint64_t)(want >> 64) && p.lo == (uint64_t)want);
    }
    {
        const uint64_t N = 1ull << 49, D = 1ull << 18;
        const uint64_t ns[] = {0, 1, 2, N - 1, N, N / 3, (N / 3) * 2, 0x1FFFFFFFFFFFFull, 0xFFFFFFFFull, 0x100000000ull};
        const uint64_t ds[] = {1, 2, 3, D - 1, D, D / 2 + 1, 255ull * 512, 257ull * 512, 65535, 65536};
        for (uint64_t n1 : ns)
            for (uint64_t d1 : ds)
                for (uint64_t n2 : ns)
                    for (uint64_t d2 : ds) {
                        const u128 l = (u128)n1 * d2, r = (u128)n2 * d1;
                        CHECK(tree_cmp_value(n1, d1, n2, d2) == (l < r ? -1 : l > r ? 1 : 0));
                    }
        for (int t = 0; t < 200000; ++t) {  // near-equal fractions: n2 / d2 one unit either side of n1 / d1 scaled
            const uint64_t d1 = 1 + below(D), d2 = 1 + below(D), n1 = below(N / D) * d1 + below(d1);
            const uint64_t n2 = (uint64_t)(((u128)n1 * d2) / d1) + below(3);
            const u128 l = (u128)n1 * d2, r = (u128)(n2 ? n2 - 1 : 0) * d1;
            CHECK(tree_cmp_value(n1, d1, n2 ? n2 - 1 : 0, d2) == (l < r ? -1 : l > r ? 1 : 0));
        }
        // the products of the bound in the header do pass 2^64
        CHECK(tree_mul_64x64((1ull << 31) * (512ull * 255) - 1, 512ull * 257).hi >= 1);
    }
    // the order, the count of rows at the minimum, the panel rules
    {
        const TreeKey none = tree_key_none(), x = tree_key(TREE_AVERAGE, 6, 2, 3, 4, 1), y = tree_key(TREE_AVERAGE, 2, 1, 2, 0, 5);
        CHECK(x.a == 1 && x.b == 4 && x.den == 6 && y.den == 2);
        CHECK(tree_key_less(x, none) && !tree_key_less(none, x) && !tree_key_less(none, none));
        CHECK(tree_key_less(y, x) && !tree_key_less(x, y));  // 6/6 = 2/2: the names decide
        CHECK(tree_key(TREE_SINGLE, 6, 2, 3, 4, 1).den == 1);
        TreeBest b = tree_best_combine(tree_best_of_row(x), tree_best_of_row(y));
        CHECK(b.rows == 2 && b.key.a == 0 && !tree_is_tied(b.rows));
        b = tree_best_combine(b, tree_best_of_row(tree_key(TREE_AVERAGE, 9, 3, 3, 7, 8)));
        CHECK(b.rows == 3 && b.key.a == 0 && tree_is_tied(b.rows));
        b = tree_best_combine(tree_best_none(), tree_best_combine(b, tree_best_of_row(tree_key(TREE_AVERAGE, 1, 1, 2, 9, 8))));
        CHECK(b.rows == 1 && b.key.a == 8 && b.key.b == 9);
        CHECK(tree_lance_williams(TREE_SINGLE, 3, 5) == 3 && tree_lance_williams(TREE_COMPLETE, 3, 5) == 5 && tree_lance_williams(TREE_AVERAGE, 3, 5) == 8);
        CHECK(tree_cache_survives(4, 1, 2) && !tree_cache_survives(1, 1, 2) && !tree_cache_survives(2, 1, 2));
        TreePanel P = tree_panel_start(1);
        CHECK(P.mrca_size == 1 && P.mrca_merge == TREE_NONE && P.largest_clade == 1);
        P = tree_panel_start(3);
        CHECK(tree_panel_merge(P, 1, 1, 2, 0) == 2 && P.largest_clade == 2 && P.mrca_size == 0);
        CHECK(tree_panel_merge(P, 2, 1, 4, 5) == 3 && P.largest_clade == 2 && P.mrca_size == 4 && P.mrca_merge == 5);
        CHECK(tree_panel_merge(P, 3, 0, 6, 7) == 3 && P.mrca_size == 4 && P.mrca_merge == 5);
    }

    uint64_t tied_seen = 0, untied_seen = 0;
    for (it = 0; it < iters; ++it) {
        const uint32_t m = 2 + (uint32_t)below(30), linkage = (uint32_t)below(3), K = (uint32_t)below(4);
        const uint64_t top = it % 5 == 0 ? (1ull << 31) - 1 : 1 + below(it % 3 == 0 ? 3 : 12);  // few distinct values: many ties
        std::vector<uint64_t> H((size_t)m * m, 0);
        for (uint32_t i = 0; i < m; ++i)
            for (uint32_t j = i + 1; j < m; ++j) H[(size_t)i * m + j] = H[(size_t)j * m + i] = it % 5 == 0 ? top - below(4) : below(top + 1);
        if (it % 11 == 3) std::fill(H.begin(), H.end(), 0ull);
        std::vector<uint8_t> cls(m, 0xFF);
        if (K)
            for (uint32_t i = 0; i < m; ++i) cls[i] = below(K + 1) < K ? (uint8_t)below(K) : 0xFF;
        // every panel non-empty: the call refuses empty ones
        for (uint32_t p = 0; p < K && p < m; ++p) cls[p] = (uint8_t)p;
        const uint32_t Ku = K < m ? K : m;
        for (uint32_t i = 0; i < m; ++i)
            if (cls[i] != 0xFF && cls[i] >= Ku) cls[i] = 0xFF;
        const TreeSerialResult R = tree_solve_serial(H.data(), m, linkage, cls.data(), Ku);
        const BruteResult B = brute(H, m, linkage, cls, Ku);
        CHECK(R.merges.size() == m - 1 && B.merges.size() == m - 1);
        uint64_t sum = 0;
        for (uint32_t i = 0; i < m; ++i)
            for (uint32_t j = i + 1; j < m; ++j) sum += H[(size_t)i * m + j];
        CHECK(R.sum_h == sum);
        for (uint32_t s = 0; s + 1 < m; ++s) {
            const TreeMerge &x = R.merges[s], &y = B.merges[s];
            CHECK(x.a == y.a && x.b == y.b && x.size_a == y.size_a && x.size_b == y.size_b && x.num == y.num && x.a < x.b);
            if (s) {  // reducible: the values never decrease
                const TreeMerge &p = R.merges[s - 1];
                const uint64_t dp = linkage == 2 ? (uint64_t)p.size_a * p.size_b : 1, dx = linkage == 2 ? (uint64_t)x.size_a * x.size_b : 1;
                CHECK((u128)p.num * dx <= (u128)x.num * dp);
            }
        }
        CHECK(R.n_zero == B.n_zero && R.n_tied == B.n_tied);
        CHECK(R.rows_recomputed >= 2ull * (m - 1));
        if (it % 11 == 3) CHECK(R.n_zero == m - 1 && R.n_tied == m - 2);
        (R.n_tied ? tied_seen : untied_seen) += 1;
        CHECK(R.panels.size() == Ku);
        for (uint32_t p = 0; p < Ku; ++p) {
            const TreePanel &x = R.panels[p], &y = B.panels[p];
            CHECK(x.n_members == y.n_members && x.largest_clade == y.largest_clade && x.mrca_size == y.mrca_size && x.mrca_merge == y.mrca_merge);
            CHECK(x.mrca_size >= x.n_members && x.largest_clade >= 1 && x.largest_clade <= x.n_members);
        }
    }
    it = -1;
    CHECK(iters < 20 || (tied_seen > 0 && untied_seen > 0));
    printf("ok %d\n", iters);
    return 0;
}
