// perm_math.h — the arithmetic of impop_permtest_scan (plain C++, no HIP types: tests/fuzz/perm_math.cc compiles it on the host
// under the sanitizers; permtest.hip runs the same comparisons on the device, pairwise_scan.hip the generator and the doubles on
// the host).  It holds the labelling generator, the four "at least as extreme" comparisons in integers, the S_nn term, the algebra
// from a quadratic form to (wa, wb), the finalisation of the record's doubles in their one operation order, and perm_window_serial:
// a whole (window, pair) as plain loops — the definition the kernels are tested against.
//
// A pair of panels k < l: the members of k u l in ascending haplotype index are POSITIONS 0 .. m - 1; a labelling z is an m-bit
// mask (bit i of word i / 64) with exactly m_k ones; z0 marks the members of k.
#pragma once
#include <stdint.h>

#include "dip_runs.h"  // DIP_HD

namespace impop {

constexpr uint32_t PERMTEST_MAX_N = 1024;      // IMPOP_PERMTEST_MAX_N
constexpr uint32_t PERMTEST_MAX_PERM = 16384;  // IMPOP_PERMTEST_MAX_PERM
constexpr uint64_t PERM_SCALE = 2952069120ull; // 720720 * 4096: every tied <= 16 divides it
typedef unsigned __int128 perm_u128;

// ---- the labellings.  sm(x) is splitmix64's output for the state x; labelling r of pair index p under `seed` draws
// u_t = sm(k3 + t * GOLDEN), t = 0, 1, .., with k1 = sm(seed), k2 = sm(k1 ^ p), k3 = sm(k2 ^ r): the standard stream started at k3.
constexpr uint64_t PERM_GOLDEN = 0x9E3779B97F4A7C15ull;
DIP_HD inline uint64_t perm_sm(uint64_t x) {
    uint64_t z = x + PERM_GOLDEN;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
DIP_HD inline uint64_t perm_key(uint64_t seed, uint32_t pair_index, uint32_t r) {
    return perm_sm(perm_sm(perm_sm(seed) ^ (uint64_t)pair_index) ^ (uint64_t)r);
}
// a partial Fisher-Yates over a[0 .. m) = 0 .. m - 1: step t = 0 .. m_a - 1 swaps a[t] with a[t + hi64(u_t * (m - t))]; the
// labelling's ones are a[0 .. m_a).  a: m words of the caller's; out: ceil(m / 64) words, overwritten.
inline void perm_labelling(uint64_t seed, uint32_t pair_index, uint32_t r, uint32_t m, uint32_t m_a, uint32_t *a, uint64_t *out) {
    const uint32_t mw = (m + 63) / 64;
    for (uint32_t i = 0; i < m; ++i) a[i] = i;
    for (uint32_t w = 0; w < mw; ++w) out[w] = 0;
    const uint64_t k3 = perm_key(seed, pair_index, r);
    for (uint32_t t = 0; t < m_a; ++t) {
        const uint64_t u = perm_sm(k3 + (uint64_t)t * PERM_GOLDEN);
        const uint32_t j = t + (uint32_t)(uint64_t)(((perm_u128)u * (perm_u128)(m - t)) >> 64);
        const uint32_t v = a[j];
        a[j] = a[t];
        a[t] = v;
        out[v >> 6] |= 1ull << (v & 63u);
    }
}

// ---- integers of a labelling
struct PermObs {
    uint64_t wa, wb, nn, tot;
};
DIP_HD inline uint64_t perm_q(uint64_t m) { return m * (m - 1) / 2 ? m * (m - 1) / 2 : 1; }  // max(m (m - 1) / 2, 1)
DIP_HD inline uint32_t perm_nn_term(uint32_t tied) { return (uint32_t)(PERM_SCALE / tied); }
// y = H z, r = H 1: 2 wa = z^T y and 2 wb = sum(r) - 2 z^T r + z^T y
DIP_HD inline void perm_wa_wb(uint64_t zHz, uint64_t zr, uint64_t sum_r, uint64_t *wa, uint64_t *wb) {
    *wa = zHz / 2;
    *wb = (sum_r - 2 * zr + zHz) / 2;
}
// x fits 63 bits and the 128-bit products cannot overflow when W_max * P_max^2 <= 2^62 (wa <= W q_k, wb <= W q_l, ab <= W m_k m_l)
DIP_HD inline bool perm_fst_admitted(uint64_t w_max, uint64_t p_max) {
    if (w_max == 0 || p_max == 0) return true;
    const perm_u128 lim = (perm_u128)1 << 62;
    const perm_u128 pp = (perm_u128)p_max * p_max;
    return pp <= lim && pp * w_max <= lim;
}
// the four one-sided tests, towards more differentiation; o = the observed labelling's integers
DIP_HD inline bool perm_ge_dxy(uint64_t wa, uint64_t wb, const PermObs &o) { return o.tot - wa - wb >= o.tot - o.wa - o.wb; }
DIP_HD inline bool perm_ge_phi(uint64_t wa, uint64_t wb, const PermObs &o, uint64_t m_k, uint64_t m_l) {
    return (perm_u128)wa * m_l + (perm_u128)wb * m_k <= (perm_u128)o.wa * m_l + (perm_u128)o.wb * m_k;
}
DIP_HD inline bool perm_ge_fst(uint64_t wa, uint64_t wb, const PermObs &o, uint64_t m_k, uint64_t m_l) {
    const uint64_t qk = perm_q(m_k), ql = perm_q(m_l);
    const uint64_t x = wa * ql + wb * qk, x0 = o.wa * ql + o.wb * qk;
    return (perm_u128)x * (o.tot - o.wa - o.wb) <= (perm_u128)x0 * (o.tot - wa - wb);
}
DIP_HD inline bool perm_ge_snn(uint64_t nn, const PermObs &o) { return nn >= o.nn; }

// ---- the record's doubles, on the host, each in its one operation order
struct PermDoubles {
    double fst, phi_st, dxy;
};
inline PermDoubles perm_doubles(const PermObs &o, uint64_t m_k, uint64_t m_l) {
    PermDoubles d;
    const uint64_t ab = o.tot - o.wa - o.wb, m = m_k + m_l;
    d.dxy = (double)ab / ((double)m_k * (double)m_l);
    const double pi_a = m_k >= 2 ? (double)o.wa / (double)perm_q(m_k) : 0.0;
    const double pi_b = m_l >= 2 ? (double)o.wb / (double)perm_q(m_l) : 0.0;
    const double pi_xy = (pi_a + pi_b) / 2.0;
    d.fst = d.dxy > 0.0 ? (d.dxy - pi_xy) / d.dxy : 0.0;
    d.phi_st = __builtin_nan("");
    if (m > 2) {
        const double ssd_w = (double)o.wa / (double)m_k + (double)o.wb / (double)m_l;
        const double ssd_a = (double)o.tot / (double)m - ssd_w;
        const double ms_w = ssd_w / (double)(m - 2);
        const double n0 = 2.0 * (double)m_k * (double)m_l / (double)m;
        const double s2a = (ssd_a - ms_w) / n0;
        const double den = s2a + ms_w;
        if (den != 0.0) d.phi_st = s2a / den;
    }
    return d;
}
// st[i] = same_i(z0) << 16 | tied_i, i in ascending haplotype index: impop_pairdist_scan's snn
inline double perm_snn(const uint32_t *st, uint32_t m) {
    double sum = 0.0;
    for (uint32_t i = 0; i < m; ++i) sum += (double)(st[i] >> 16) / (double)(st[i] & 0xFFFFu);
    return sum / (double)m;
}
inline double perm_p(uint32_t ge, uint32_t n_perm) { return (1.0 + (double)ge) / ((double)n_perm + 1.0); }

// ---- a whole (window, pair) as loops.  H: m x m, symmetric, zero diagonal.  z0 and labels[r] are masks of mw = ceil(m / 64)
// words.  st: m words (above); null (nullable): n_perm x {wa, wb, nn}; ge: fst, phi, dxy, snn.
DIP_HD inline bool perm_bit(const uint64_t *z, uint32_t i) { return (z[i >> 6] >> (i & 63u)) & 1u; }
inline void perm_labelling_serial(const uint32_t *H, uint32_t m, const uint64_t *z, uint64_t *wa, uint64_t *wb, uint64_t *nn,
                                  uint32_t *st) {
    uint64_t a = 0, b = 0, n = 0;
    for (uint32_t i = 0; i < m; ++i) {
        uint32_t d = 0xFFFFFFFFu, tied = 0, same = 0;
        for (uint32_t j = 0; j < m; ++j) {
            if (j == i) continue;
            const uint32_t h = H[(uint64_t)i * m + j];
            if (j > i && perm_bit(z, i) == perm_bit(z, j)) (perm_bit(z, i) ? a : b) += h;
            if (h < d) { d = h; tied = 0; same = 0; }
            if (h == d) { ++tied; same += perm_bit(z, i) == perm_bit(z, j) ? 1u : 0u; }
        }
        n += (uint64_t)same * perm_nn_term(tied);
        if (st) st[i] = same << 16 | tied;
    }
    *wa = a; *wb = b; *nn = n;
}
inline void perm_window_serial(const uint32_t *H, uint32_t m, uint32_t m_k, const uint64_t *z0, const uint64_t *labels, uint32_t n_perm,
                               PermObs *obs, uint32_t *st, uint32_t ge[4], uint64_t *null) {
    const uint32_t mw = (m + 63) / 64;
    PermObs o;
    o.tot = 0;
    for (uint32_t i = 0; i < m; ++i)
        for (uint32_t j = i + 1; j < m; ++j) o.tot += H[(uint64_t)i * m + j];
    perm_labelling_serial(H, m, z0, &o.wa, &o.wb, &o.nn, st);
    ge[0] = ge[1] = ge[2] = ge[3] = 0;
    for (uint32_t r = 0; r < n_perm; ++r) {
        uint64_t wa, wb, nn;
        perm_labelling_serial(H, m, labels + (uint64_t)r * mw, &wa, &wb, &nn, nullptr);
        ge[0] += perm_ge_fst(wa, wb, o, m_k, m - m_k) ? 1u : 0u;
        ge[1] += perm_ge_phi(wa, wb, o, m_k, m - m_k) ? 1u : 0u;
        ge[2] += perm_ge_dxy(wa, wb, o) ? 1u : 0u;
        ge[3] += perm_ge_snn(nn, o) ? 1u : 0u;
        if (null) { null[3 * (uint64_t)r] = wa; null[3 * (uint64_t)r + 1] = wb; null[3 * (uint64_t)r + 2] = nn; }
    }
    *obs = o;
}

}  // namespace impop
