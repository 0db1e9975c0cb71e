// tree_math.h — the arithmetic of impop_tree_scan's agglomerative clustering (plain C++, no HIP types: tests/fuzz/tree_math.cc
// compiles it on the host under the sanitizers; tree.hip runs the same functions on the device).
//
// A step merges the live pair of clusters with the smallest (value, a, b), a < b the clusters' names (lowest member position).  The
// value of a pair is a fraction num / den: den = 1 for single and complete linkage, |A| |B| for average linkage, where num is the
// SUM of the distances over A x B.  Values are compared exactly (tree_cmp_value: 128-bit cross products), never as doubles.
// Nobody rescans the matrix per step: every live row k keeps its nearest neighbour nn[k] under the same order (over ALL other
// live clusters, so the pair a step merges is cached by both of its rows).  After the merge (a, b) -> a, with the matrix row a
// rewritten by Lance-Williams, row k != a, b keeps its cache unless it pointed at a or b (tree_cache_survives), after comparing
// the one new entry (k, a) with it: all three linkages are reducible, d(k, a u b) >= min(d(k, a), d(k, b)), so no other entry of
// row k can have moved below the cached one — the new entry can only win by the tie rule (equal value, a < nn[k]).
// The steps over rows — the argmin over the cached neighbours, the rescans — are the caller's: the kernel spreads them over a
// workgroup, tree_solve_serial runs them as plain loops.
#pragma once
#include <stdint.h>

#include <vector>

#include "dip_runs.h"  // DIP_HD

#define TREE_FN DIP_HD inline __attribute__((always_inline))

namespace impop {

constexpr uint32_t TREE_MAX_N = 1024;  // IMPOP_TREE_MAX_N
constexpr uint32_t TREE_MAX_POP = 8;
constexpr uint32_t TREE_SINGLE = 0, TREE_COMPLETE = 1, TREE_AVERAGE = 2;  // IMPOP_LINKAGE_*
constexpr uint32_t TREE_NONE = 0xFFFFFFFFu;

// ---- exact comparison of two values n1 / d1 and n2 / d2 (d > 0): the sign of n1 d2 - n2 d1 from the full 128-bit products.
// num <= W |A| |B| < 2^31 2^18 and, for two pairs live at once, den1 den2 <= m^4 / 64 = 2^34 (|A|^2 |B| |C| with |A| + |B| + |C|
// <= m = 1024, at |A| = m / 2), so a product reaches 2^65: 64 bits do not hold it.
struct TreeU128 {
    uint64_t hi, lo;
};
TREE_FN TreeU128 tree_mul_64x64(uint64_t x, uint64_t y) {
    const uint64_t x0 = (uint32_t)x, x1 = x >> 32, y0 = (uint32_t)y, y1 = y >> 32;
    const uint64_t p00 = x0 * y0, p01 = x0 * y1, p10 = x1 * y0, p11 = x1 * y1;
    const uint64_t mid = (p00 >> 32) + (uint32_t)p01 + (uint32_t)p10;  // < 3 * 2^32
    return TreeU128{p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32), (mid << 32) | (uint32_t)p00};
}
TREE_FN int tree_cmp_value(uint64_t n1, uint64_t d1, uint64_t n2, uint64_t d2) {
    if (d1 == d2) return n1 < n2 ? -1 : n1 > n2 ? 1 : 0;
    const TreeU128 l = tree_mul_64x64(n1, d2), r = tree_mul_64x64(n2, d1);
    if (l.hi != r.hi) return l.hi < r.hi ? -1 : 1;
    return l.lo < r.lo ? -1 : l.lo > r.lo ? 1 : 0;
}

// ---- a live pair of clusters as the order sees it; a == TREE_NONE: no pair
struct TreeKey {
    uint64_t num;
    uint32_t den, a, b;
};
TREE_FN TreeKey tree_key_none() { return TreeKey{0ull, 1u, TREE_NONE, TREE_NONE}; }
// the pair of the clusters named k and j (k != j), their matrix entry x (min / max / sum over the two clusters) and sizes
TREE_FN TreeKey tree_key(uint32_t linkage, uint64_t x, uint32_t size_k, uint32_t size_j, uint32_t k, uint32_t j) {
    return TreeKey{x, linkage == TREE_AVERAGE ? size_k * size_j : 1u, k < j ? k : j, k < j ? j : k};
}
// THE order: (value, a, b) lexicographic; a pair precedes no pair
TREE_FN bool tree_key_less(const TreeKey &x, const TreeKey &y) {
    if (x.a == TREE_NONE) return false;
    if (y.a == TREE_NONE) return true;
    const int c = tree_cmp_value(x.num, x.den, y.num, y.den);
    if (c) return c < 0;
    return x.a != y.a ? x.a < y.a : x.b < y.b;
}

// ---- the argmin over the rows' cached neighbours, with the number of ROWS that attain the minimum value: the pair a step merges
// is cached by its two rows, so three or more rows at the minimum <=> at least two live pairs attain it (two pairs that share a
// cluster put three rows there, two disjoint pairs four)
struct TreeBest {
    TreeKey key;
    uint32_t rows;
};
TREE_FN TreeBest tree_best_none() { return TreeBest{tree_key_none(), 0u}; }
TREE_FN TreeBest tree_best_of_row(const TreeKey &key) { return TreeBest{key, key.a == TREE_NONE ? 0u : 1u}; }
TREE_FN TreeBest tree_best_combine(const TreeBest &x, const TreeBest &y) {
    if (x.key.a == TREE_NONE) return y;
    if (y.key.a == TREE_NONE) return x;
    const int c = tree_cmp_value(x.key.num, x.key.den, y.key.num, y.key.den);
    if (c) return c < 0 ? x : y;
    TreeBest r = tree_key_less(y.key, x.key) ? y : x;
    r.rows = x.rows + y.rows;
    return r;
}
TREE_FN bool tree_is_tied(uint32_t rows_at_minimum) { return rows_at_minimum >= 3u; }

// ---- Lance-Williams in integers: the entry (k, a u b) from the entries (k, a) and (k, b)
TREE_FN uint64_t tree_lance_williams(uint32_t linkage, uint64_t x_ka, uint64_t x_kb) {
    if (linkage == TREE_SINGLE) return x_ka < x_kb ? x_ka : x_kb;
    if (linkage == TREE_COMPLETE) return x_ka > x_kb ? x_ka : x_kb;
    return x_ka + x_kb;
}
// does row k's cached nearest neighbour survive the merge (a, b) -> a?  (Behind it the one new entry (k, a) is still compared.)
TREE_FN bool tree_cache_survives(uint32_t nn_k, uint32_t a, uint32_t b) { return nn_k != a && nn_k != b; }

// ---- records
struct TreeMerge {  // impop_tree_merge
    uint32_t a, b, size_a, size_b;
    uint64_t num;
};
struct TreePanel {  // impop_tree_panel
    uint32_t n_members, largest_clade, mrca_size, mrca_merge;
};
// a panel before the first merge: its members are singletons (clades of size 1); a one-member panel is its own ancestor
TREE_FN TreePanel tree_panel_start(uint32_t n_members) { return TreePanel{n_members, 1u, n_members == 1u ? 1u : 0u, TREE_NONE}; }
// merge number `step` forms a cluster of size_ab members: in_a + in_b of them are the panel's.  -> the merged cluster's count
TREE_FN uint32_t tree_panel_merge(TreePanel &P, uint32_t in_a, uint32_t in_b, uint32_t size_ab, uint32_t step) {
    const uint32_t in_ab = in_a + in_b;
    if (in_ab == size_ab && size_ab > P.largest_clade) P.largest_clade = size_ab;
    if (P.mrca_size == 0u && in_ab == P.n_members) {
        P.mrca_size = size_ab;
        P.mrca_merge = step;
    }
    return in_ab;
}
// the window's two merge counters
TREE_FN void tree_count_merge(uint64_t num, uint32_t rows_at_minimum, uint32_t &n_zero, uint32_t &n_tied) {
    n_zero += num == 0ull ? 1u : 0u;
    n_tied += tree_is_tied(rows_at_minimum) ? 1u : 0u;
}

// ---- the whole clustering of one window, serially, over a full symmetric m x m matrix of distances (the scheme of the kernel:
// cached neighbours, rescans of the invalidated rows only).  cls: the panel of every position, 0xFF = none (nullable with K = 0).
struct TreeSerialResult {
    std::vector<TreeMerge> merges;
    std::vector<TreePanel> panels;
    uint32_t n_zero = 0, n_tied = 0;
    uint64_t sum_h = 0, rows_recomputed = 0;
};
inline TreeKey tree_scan_row_serial(const std::vector<uint64_t> &S, const std::vector<uint32_t> &size, uint32_t m, uint32_t linkage, uint32_t k) {
    TreeKey best = tree_key_none();
    for (uint32_t j = 0; j < m; ++j) {
        if (j == k || !size[j]) continue;
        const TreeKey key = tree_key(linkage, S[(size_t)k * m + j], size[k], size[j], k, j);
        if (tree_key_less(key, best)) best = key;
    }
    return best;
}
inline TreeSerialResult tree_solve_serial(const uint64_t *H, uint32_t m, uint32_t linkage, const uint8_t *cls, uint32_t K) {
    TreeSerialResult R;
    std::vector<uint64_t> S(H, H + (size_t)m * m), val(m, 0);
    std::vector<uint32_t> size(m, 1u), nn(m, TREE_NONE), cnt((size_t)K * m, 0u), psize(K, 0u);
    for (uint32_t i = 0; i < m; ++i) {
        for (uint32_t j = i + 1; j < m; ++j) R.sum_h += H[(size_t)i * m + j];
        if (K && cls[i] < K) { cnt[(size_t)cls[i] * m + i] = 1u; ++psize[cls[i]]; }
    }
    for (uint32_t p = 0; p < K; ++p) R.panels.push_back(tree_panel_start(psize[p]));
    auto rescan = [&](uint32_t k) {
        const TreeKey key = tree_scan_row_serial(S, size, m, linkage, k);
        nn[k] = key.a == TREE_NONE ? TREE_NONE : key.a == k ? key.b : key.a;
        val[k] = key.num;
    };
    for (uint32_t k = 0; k < m; ++k) rescan(k);
    for (uint32_t step = 0; step + 1 < m; ++step) {
        TreeBest best = tree_best_none();
        for (uint32_t k = 0; k < m; ++k)
            if (size[k] && nn[k] != TREE_NONE)
                best = tree_best_combine(best, tree_best_of_row(tree_key(linkage, val[k], size[k], size[nn[k]], k, nn[k])));
        const uint32_t a = best.key.a, b = best.key.b, sa = size[a], sb = size[b];
        R.merges.push_back(TreeMerge{a, b, sa, sb, best.key.num});
        tree_count_merge(best.key.num, best.rows, R.n_zero, R.n_tied);
        std::vector<uint32_t> again = {a};
        for (uint32_t k = 0; k < m; ++k) {
            if (!size[k] || k == a || k == b) continue;
            const uint64_t x = tree_lance_williams(linkage, S[(size_t)a * m + k], S[(size_t)b * m + k]);
            S[(size_t)a * m + k] = S[(size_t)k * m + a] = x;
            if (!tree_cache_survives(nn[k], a, b)) again.push_back(k);
            else if (tree_key_less(tree_key(linkage, x, size[k], sa + sb, k, a), tree_key(linkage, val[k], size[k], size[nn[k]], k, nn[k]))) {
                nn[k] = a;
                val[k] = x;
            }
        }
        size[a] = sa + sb;
        size[b] = 0;
        for (uint32_t p = 0; p < K; ++p)
            cnt[(size_t)p * m + a] = tree_panel_merge(R.panels[p], cnt[(size_t)p * m + a], cnt[(size_t)p * m + b], sa + sb, step);
        R.rows_recomputed += again.size() + 1;  // + row b, which pointed at a and retires
        for (uint32_t k : again) rescan(k);
    }
    return R;
}

}  // namespace impop
