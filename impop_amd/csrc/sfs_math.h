// sfs_math.h — the host arithmetic of impop_sfs_scan (sfs.hip), each expression once: the eight doubles of a record from its
// integers, how the table pass cuts a window's tile range into parts, and where a table lies in a window's row of tables.
// Plain C++, no HIP: tests/fuzz/sfs_host.cc compiles it on the host under the sanitizers and checks the part cutter and the
// offsets against a brute-force model; tests/plain_sfs.py restates the doubles in the same operator order (the build's
// -ffp-contract=off keeps every product and sum a rounding of its own, so the two agree bit for bit).
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

namespace impop {

// What the doubles of a record need of n alone, formed once per population: every member is a whole subexpression of the
// header's formulas, so taking it from here gives the bits the formula written out gives.  a1, a2, e1, e2: Tajima's constants
// for n (tajima_consts, device_utils.h).
struct SfsConsts {
    uint32_t n;
    double a1, e1, e2;
    double P;        // n (n - 1) / 2
    double nm1;      // n - 1
    double t2_den;   // a1^2 + a2
    double h_w, h_t2;  // var_H = h_w theta_w + h_t2 T2 (Zeng et al. 2006, eq. 14: Var[theta_pi - theta_L])
    double e_w, e_t2;  // var_E = e_w theta_w + e_t2 T2 (eq. 12: Var[theta_L - theta_W])
};
inline SfsConsts sfs_consts(uint32_t n, double a1, double a2, double e1, double e2) {
    SfsConsts c;
    const double dn = (double)n;
    c.n = n;
    c.a1 = a1; c.e1 = e1; c.e2 = e2;
    c.P = dn * (dn - 1.0) / 2.0;
    c.nm1 = dn - 1.0;
    c.t2_den = a1 * a1 + a2;
    const double b = a2 + 1.0 / (dn * dn);
    c.h_w = (dn - 2.0) / (6.0 * (dn - 1.0));
    c.h_t2 = (18.0 * dn * dn * (3.0 * dn + 2.0) * b - (88.0 * dn * dn * dn + 9.0 * dn * dn - 13.0 * dn + 6.0)) /
             (9.0 * dn * (dn - 1.0) * (dn - 1.0));
    c.e_w = dn / (2.0 * (dn - 1.0)) - 1.0 / a1;
    c.e_t2 = a2 / (a1 * a1) + 2.0 * (dn / (dn - 1.0)) * (dn / (dn - 1.0)) * a2 - 2.0 * (dn * a2 - dn + 1.0) / ((dn - 1.0) * a1) -
             (3.0 * dn + 1.0) / (dn - 1.0);
    return c;
}

// out[8] = theta_w, theta_pi, theta_h, theta_l, tajima_d, faywu_h, faywu_h_norm, zeng_e (include/impop_hip.h has the definitions)
// of a population of c.n sequences.  n < 2: eight NaN.
inline void sfs_neutrality(const SfsConsts &c, uint64_t seg, uint64_t sum_het, uint64_t sum_c, uint64_t sum_c2, double out[8]) {
    const double nan = __builtin_nan("");
    if (c.n < 2) {
        for (int i = 0; i < 8; ++i) out[i] = nan;
        return;
    }
    const double S = (double)seg;
    // a ratio is undefined without segregating sites and where its variance is not a positive finite number
    auto ratio = [&](double num, double var) { return (S > 0.0 && var > 0.0 && __builtin_isfinite(var)) ? num / __builtin_sqrt(var) : nan; };
    const double theta_w = S / c.a1;
    const double theta_pi = (double)sum_het / c.P;
    const double theta_h = (double)sum_c2 / c.P;
    const double theta_l = (double)sum_c / c.nm1;
    const double var_d = c.e1 * S + c.e2 * S * (S - 1.0);
    const double T2 = S * (S - 1.0) / c.t2_den;
    const double var_h = c.h_w * theta_w + c.h_t2 * T2;
    const double var_e = c.e_w * theta_w + c.e_t2 * T2;
    out[0] = theta_w; out[1] = theta_pi; out[2] = theta_h; out[3] = theta_l;
    out[4] = ratio(theta_pi - theta_w, var_d);
    out[5] = theta_pi - theta_h;
    out[6] = ratio(theta_pi - theta_l, var_h);
    out[7] = ratio(theta_l - theta_w, var_e);
}

// ---- the table pass: a workgroup owns one (window, part) item, a part being a run of the window's tile range
struct SfsItem {
    uint32_t win;     // the window, counted from the first window of the chunk
    uint32_t t0, t1;  // its tiles [t0, t1), a part of the window's range
};
// The windows [w_begin, w_end) of `wins` (anything with a tile range t0, t1) cut into items of at most part_tiles tiles, in equal
// shares (a 9-tile window under a limit of 4 becomes 3 + 3 + 3): every tile of every window lies in exactly one item, in order; a
// window without tiles gets none (its tables stay zero).
template <typename Win>
inline void sfs_cut_parts(const Win *wins, uint64_t w_begin, uint64_t w_end, uint32_t part_tiles, std::vector<SfsItem> &items) {
    if (part_tiles < 1) part_tiles = 1;
    for (uint64_t w = w_begin; w < w_end; ++w) {
        const uint64_t t0 = wins[w].t0, nt = wins[w].t1 > t0 ? wins[w].t1 - t0 : 0;
        if (!nt) continue;
        const uint64_t n_parts = (nt + part_tiles - 1) / part_tiles, per = (nt + n_parts - 1) / n_parts;
        for (uint64_t s = 0; s < nt; s += per)
            items.push_back({(uint32_t)(w - w_begin), (uint32_t)(t0 + s), (uint32_t)(t0 + (s + per < nt ? s + per : nt))});
    }
}
// the items sfs_cut_parts makes of a window of nt tiles
inline uint64_t sfs_part_count(uint64_t nt, uint32_t part_tiles) {
    if (part_tiles < 1) part_tiles = 1;
    if (!nt) return 0;
    const uint64_t n_parts = (nt + part_tiles - 1) / part_tiles, per = (nt + n_parts - 1) / n_parts;
    return (nt + per - 1) / per;
}

// ---- where the tables lie.  A window's row of 1-D spectra concatenates the K populations' n_k + 1 bins; its row of joint
// spectra concatenates the pairs' (n_a + 1) x (n_b + 1) tables, row-major in c_a.
struct SfsTableRows {
    std::vector<uint64_t> sfs_off;   // K + 1: population k's spectrum starts at sfs_off[k]; sfs_off[K] = the row's length
    std::vector<uint64_t> jsfs_off;  // n_pairs + 1, likewise
};
inline SfsTableRows sfs_table_rows(const uint32_t *nk, uint32_t K, const uint32_t *pairs, uint32_t n_pairs) {
    SfsTableRows r;
    r.sfs_off.assign(1, 0);
    for (uint32_t k = 0; k < K; ++k) r.sfs_off.push_back(r.sfs_off.back() + (uint64_t)nk[k] + 1);
    r.jsfs_off.assign(1, 0);
    for (uint32_t p = 0; p < n_pairs; ++p)
        r.jsfs_off.push_back(r.jsfs_off.back() + ((uint64_t)nk[pairs[2 * p]] + 1) * ((uint64_t)nk[pairs[2 * p + 1]] + 1));
    return r;
}
// the bin of the joint table of sizes (n_a, n_b) that the counts (c_a, c_b) fall in
inline uint64_t sfs_joint_bin(uint32_t c_a, uint32_t c_b, uint32_t n_b) { return (uint64_t)c_a * ((uint64_t)n_b + 1) + c_b; }

}  // namespace impop
