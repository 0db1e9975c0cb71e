// pairdist_math.h — the integer combines and the record finalisation of impop_pairdist_scan (plain C++, no HIP types:
// tests/fuzz/pairdist_math.cc compiles it on the host under the sanitizers; pairdist.hip runs the same code on the device).
//
// A window's panels are laid out back to back as POSITIONS 0 .. M - 1 (M <= 4096): panel k holds positions off[k] .. off[k + 1),
// each panel in ascending haplotype index.  Inside one record the pairs (pi, pj) are ordered by position exactly as the contract
// orders them by haplotype index — (i, j) with i < j of a panel, or i from panel k and j from panel l > k — so the extremes are
// reduced as packed keys over positions and mapped to haplotype indexes only when the record is written.
#pragma once
#include <stdint.h>

#include "dip_runs.h"  // DIP_HD

namespace impop {

constexpr uint32_t PAIRDIST_MAX_N = 4096;  // IMPOP_PAIRDIST_MAX_N: positions fit 12 bits
constexpr uint32_t PAIRDIST_NONE = 0xFFFFFFFFu;

// ---- the key order.  min: the smallest key = the smallest H, then the smallest pi, then the smallest pj.  max: the LARGEST key =
// the largest H, then the smallest pi, then the smallest pj (the position part is stored complemented).
DIP_HD inline uint32_t pd_pos_pair(uint32_t pi, uint32_t pj) { return (pi << 16) | pj; }
DIP_HD inline uint64_t pd_min_key(uint32_t h, uint32_t pi, uint32_t pj) { return ((uint64_t)h << 32) | pd_pos_pair(pi, pj); }
DIP_HD inline uint64_t pd_max_key(uint32_t h, uint32_t pi, uint32_t pj) { return ((uint64_t)h << 32) | (0xFFFFFFFFu - pd_pos_pair(pi, pj)); }
constexpr uint64_t PD_MIN_EMPTY = 0xFFFFFFFFFFFFFFFFull;  // above every real key (H <= 2^31)
constexpr uint64_t PD_MAX_EMPTY = 0ull;                   // below every real key (a position pair is < 2^28)

// ---- the sums and extremes of a set of pairs
struct DistAcc {
    uint64_t sum_h, sum_h2, n_zero, min_key, max_key;
};
DIP_HD inline DistAcc pd_acc_empty() { return DistAcc{0ull, 0ull, 0ull, PD_MIN_EMPTY, PD_MAX_EMPTY}; }
DIP_HD inline void pd_acc_add(DistAcc &a, uint32_t h, uint32_t pi, uint32_t pj) {
    a.sum_h += h;
    a.sum_h2 += (uint64_t)h * h;
    a.n_zero += h == 0 ? 1u : 0u;
    const uint64_t lo = pd_min_key(h, pi, pj), hi = pd_max_key(h, pi, pj);
    if (lo < a.min_key) a.min_key = lo;
    if (hi > a.max_key) a.max_key = hi;
}
DIP_HD inline DistAcc pd_acc_merge(const DistAcc &a, const DistAcc &b) {
    return DistAcc{a.sum_h + b.sum_h, a.sum_h2 + b.sum_h2, a.n_zero + b.n_zero, a.min_key < b.min_key ? a.min_key : b.min_key,
                   a.max_key > b.max_key ? a.max_key : b.max_key};
}

// ---- a member's nearest neighbours inside ONE panel: the smallest H and how many of the panel attain it
struct DistNN {
    uint32_t min_h, ties;  // ties 0: nothing seen (min_h = PAIRDIST_NONE)
};
DIP_HD inline DistNN pd_nn_empty() { return DistNN{PAIRDIST_NONE, 0u}; }
DIP_HD inline void pd_nn_add(DistNN &a, uint32_t h) {
    if (h < a.min_h) { a.min_h = h; a.ties = 1; }
    else if (h == a.min_h) a.ties += 1;
}
DIP_HD inline DistNN pd_nn_merge(const DistNN &a, const DistNN &b) {
    if (a.ties == 0) return b;
    if (b.ties == 0) return a;
    if (a.min_h != b.min_h) return a.min_h < b.min_h ? a : b;
    return DistNN{a.min_h, a.ties + b.ties};
}
// ... and inside the union of its own panel (itself excluded) and another: tied_i and same_i of the contract
DIP_HD inline void pd_nn_pair(const DistNN &own, const DistNN &other, uint32_t *tied, uint32_t *same) {
    const DistNN u = pd_nn_merge(own, other);
    *tied = u.ties;
    *same = (own.ties != 0 && own.min_h == u.min_h) ? own.ties : 0u;
}

// ---- the two doubles, in their one operation order
DIP_HD inline double pd_snn_term(uint32_t same, uint32_t tied) { return (double)same / (double)tied; }
DIP_HD inline double pd_snn_finish(double sum, uint32_t m_both) { return sum / (double)m_both; }
DIP_HD inline double pd_gmin(uint32_t min_h, uint64_t sum_h, uint64_t n_pairs) {
    if (sum_h == 0) return __builtin_nan("");
    return (double)min_h / ((double)sum_h / (double)n_pairs);
}

// ---- sum_h2 is exact when W_max^2 * P_max <= 2^64 - 1
DIP_HD inline bool pd_sum_h2_admitted(uint64_t w_max, uint64_t p_max) {
    if (w_max == 0 || p_max == 0) return true;
    if (w_max > 0xFFFFFFFFull) return false;  // W^2 >= 2^64
    return w_max * w_max <= 0xFFFFFFFFFFFFFFFFull / p_max;
}

// ---- the records' shared distance fields from an accumulator; hap_of: haplotype index of a position
struct DistFields {
    uint64_t sum_h, sum_h2, n_zero;
    uint32_t min_h, max_h, min_i, min_j, max_i, max_j;
};
DIP_HD inline DistFields pd_fields(const DistAcc &a, uint64_t n_pairs, const uint32_t *hap_of) {
    DistFields f;
    f.sum_h = a.sum_h; f.sum_h2 = a.sum_h2; f.n_zero = a.n_zero;
    if (n_pairs == 0) {
        f.min_h = f.max_h = 0;
        f.min_i = f.min_j = f.max_i = f.max_j = PAIRDIST_NONE;
        return f;
    }
    const uint32_t lo = (uint32_t)a.min_key, hi = 0xFFFFFFFFu - (uint32_t)a.max_key;
    f.min_h = (uint32_t)(a.min_key >> 32); f.max_h = (uint32_t)(a.max_key >> 32);
    f.min_i = hap_of[lo >> 16]; f.min_j = hap_of[lo & 0xFFFFu];
    f.max_i = hap_of[hi >> 16]; f.max_j = hap_of[hi & 0xFFFFu];
    return f;
}

// index of the pair of panels a < b among K, in impop_scan_multi's order (0,1),(0,2),..,(1,2),..
DIP_HD inline uint32_t pd_pair_index(uint32_t K, uint32_t a, uint32_t b) { return a * (2u * K - a - 1u) / 2u + (b - a - 1u); }

// the bin of a distance: the last bin collects the overflow
DIP_HD inline uint32_t pd_bin(uint32_t h, uint32_t width, uint32_t bins) {
    const uint32_t b = h / width;
    return b < bins - 1u ? b : bins - 1u;
}

}  // namespace impop
