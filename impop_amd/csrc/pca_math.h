// pca_math.h — the arithmetic of impop_pca_scan's block subspace iteration (plain C++, no HIP types: tests/fuzz/pca_math.cc
// compiles it on the host under the sanitizers; pca.hip runs the same functions on the device).
//
// The iteration keeps a block V of PCA_B = 16 columns over the m members, orthonormal and orthogonal to the ones vector (unused
// columns, m - 1 < 16, are zero).  One step: Z = B V = -1/2 J (H V); G = V^T Z (16 x 16, symmetric); G = Q diag(theta) Q^T by
// Jacobi rotations in the fixed round-robin order below; X = V Q are the Ritz vectors, Z Q = B X, and the residual of pair j is
// || (Z Q)_j - theta_j X_j ||_2; unless the first `rank` pairs pass the convergence rule, V <- orthonormalise(Z Q) and again.
// Everything a ROW of the block needs is a function of that row here (a thread of the kernel owns rows); the sums over rows
// between them are the caller's: the kernel reduces them over a workgroup in one fixed order, pca_solve_serial with plain loops.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "dip_runs.h"  // DIP_HD

#define PCA_FN DIP_HD inline __attribute__((always_inline))

namespace impop {

constexpr uint32_t PCA_MAX_N = 1024;  // IMPOP_PCA_MAX_N
constexpr uint32_t PCA_MAX_K = 8;     // IMPOP_PCA_MAX_K
constexpr int PCA_B = 16;             // columns of the block: at least k + 8 for every k
constexpr int PCA_MAX_SWEEPS = 30;
constexpr uint32_t PCA_FLAG_UNCONVERGED = 1u;

// columns in use: the centred space has m - 1 dimensions
PCA_FN uint32_t pca_block_cols(uint32_t m) { return m - 1u < (uint32_t)PCA_B ? m - 1u : (uint32_t)PCA_B; }

// ---- the start block: a fixed function of (member position, column) in [-1, 1), zero in the unused columns
PCA_FN double pca_start(uint32_t pos, uint32_t col, uint32_t cols) {
    if (col >= cols) return 0.0;
    uint64_t x = (((uint64_t)pos << 8) | col) * 0x9E3779B97F4A7C15ull + 0xD1B54A32D192ED03ull;
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return (double)(x >> 11) * (1.0 / 4503599627370496.0) - 1.0;
}

// ---- Z = -1/2 J (H V), a row at a time: y += h * (row j of V) for every member j, then the column means come off
PCA_FN void pca_hv_add(double (&y)[PCA_B], double h, const double *v, uint32_t stride) {
    for (int c = 0; c < PCA_B; ++c) y[c] = fma(h, v[(size_t)c * stride], y[c]);
}
PCA_FN double pca_mean(double sum, uint32_t m) { return sum / (double)m; }
PCA_FN void pca_bv_row(double (&y)[PCA_B], const double *mean) {
    for (int c = 0; c < PCA_B; ++c) y[c] = -0.5 * (y[c] - mean[c]);
}
PCA_FN void pca_centre_row(double (&z)[PCA_B], const double *mean) {
    for (int c = 0; c < PCA_B; ++c) z[c] = z[c] - mean[c];
}

// ---- orthonormalisation: classical Gram-Schmidt, twice, column by column.  Per column j: p[i] += z_i z_j (i <= j; p[j] is the
// squared norm) summed over the rows; z_j -= sum_{i<j} p[i] z_i; the same once more; the squared norm again; scale.
PCA_FN void pca_gs_partials(const double (&z)[PCA_B], int j, double (&p)[PCA_B]) {
    for (int i = 0; i <= j; ++i) p[i] += z[i] * z[j];
}
PCA_FN double pca_sq(double x) { return x * x; }
PCA_FN void pca_gs_subtract(double (&z)[PCA_B], int j, const double *dots) {
    double s = 0.0;
    for (int i = 0; i < j; ++i) s += dots[i] * z[i];
    z[j] -= s;
}
// a column that is zero, not finite, or cancelled to nothing against the columns before it (the block has run out of range:
// rank B < 16) becomes a zero column: it then stays zero, its Ritz value is exactly 0
PCA_FN double pca_gs_scale(double n_before, double n_after) {
    if (!(n_after > 0.0) || !(n_before < INFINITY) || !(n_after > n_before * 7.888609052210118e-31 /* 2^-100 */)) return 0.0;
    return 1.0 / sqrt(n_after);
}

// ---- Rayleigh-Ritz: p[c] += v_i z_c over the rows gives row i of G; the block times Q, a row at a time
PCA_FN void pca_dot_partials(double vi, const double (&z)[PCA_B], double (&p)[PCA_B]) {
    for (int c = 0; c < PCA_B; ++c) p[c] += vi * z[c];
}
PCA_FN void pca_rotate_row(const double (&z)[PCA_B], const double *Q /* 16 x 16, row-major */, double (&out)[PCA_B]) {
    for (int c = 0; c < PCA_B; ++c) out[c] = 0.0;
    for (int d = 0; d < PCA_B; ++d)
        for (int c = 0; c < PCA_B; ++c) out[c] = fma(z[d], Q[d * PCA_B + c], out[c]);
}
PCA_FN void pca_resid_partials(const double (&zq)[PCA_B], const double (&x)[PCA_B], const double *theta, double (&p)[PCA_B]) {
    for (int c = 0; c < PCA_B; ++c) {
        const double d = zq[c] - theta[c] * x[c];
        p[c] += d * d;
    }
}

// ---- the 16 x 16 symmetric eigensolver: cyclic Jacobi, the 120 pairs of a sweep in 15 rounds of 8 disjoint pairs (round-robin:
// index 15 meets index r in round r, the others pair up around it), so that a round's rotations commute and every element of
// A' = J^T A J and Q' = Q J is a function of four old elements.  A rotation is skipped when |a_pq| <= thr.
PCA_FN int pca_rr_partner(int round, int x) {
    if (x == 15) return round;
    if (x == round) return 15;
    return (2 * round - x + 30) % 15;
}
PCA_FN double pca_jacobi_threshold(const double *A) {
    double mx = 0.0;
    for (int i = 0; i < PCA_B; ++i) mx = fabs(A[i * PCA_B + i]) > mx ? fabs(A[i * PCA_B + i]) : mx;
    return mx * 1.3877787807814457e-17;  // 2^-56: below the rounding of the rotations themselves, and of any tol >= 1e-13
}
// the rotation of the pair p < q: J_pp = J_qq = c, J_pq = s, J_qp = -s annihilates a_pq
PCA_FN void pca_jacobi_angle(double app, double aqq, double apq, double thr, double *c, double *s) {
    if (!(fabs(apq) > thr)) { *c = 1.0; *s = 0.0; return; }
    const double th = (aqq - app) / (2.0 * apq);
    const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
    *c = 1.0 / sqrt(t * t + 1.0);
    *s = t * *c;
}
// cs[x] = c of x's pair; ts[x] = -s for the smaller index of the pair, +s for the larger
PCA_FN void pca_jacobi_round_angles(const double *A, double thr, int round, int x, double *cs, double *ts) {
    const int y = pca_rr_partner(round, x);
    if (x > y) return;
    double c, s;
    pca_jacobi_angle(A[x * PCA_B + x], A[y * PCA_B + y], A[x * PCA_B + y], thr, &c, &s);
    cs[x] = c; cs[y] = c; ts[x] = -s; ts[y] = s;
}
PCA_FN double pca_jacobi_elem(const double *A, const double *cs, const double *ts, int round, int i, int j) {
    if (i > j) { const int t = i; i = j; j = t; }  // one formula for both halves: A' stays exactly symmetric
    const int ip = pca_rr_partner(round, i), jp = pca_rr_partner(round, j);
    if (j == ip && ts[i] != 0.0) return 0.0;  // the annihilated element
    const double tij = cs[j] * A[i * PCA_B + j] + ts[j] * A[i * PCA_B + jp];
    const double tpj = cs[j] * A[ip * PCA_B + j] + ts[j] * A[ip * PCA_B + jp];
    return cs[i] * tij + ts[i] * tpj;
}
PCA_FN double pca_jacobi_qelem(const double *Q, const double *cs, const double *ts, int round, int a, int j) {
    return cs[j] * Q[a * PCA_B + j] + ts[j] * Q[a * PCA_B + pca_rr_partner(round, j)];
}
// descending order of the first `cols` diagonal entries, the lower index first on ties; the unused ones stay behind them
PCA_FN void pca_sort_desc(const double *A, uint32_t cols, int *order) {
    for (int i = 0; i < PCA_B; ++i) order[i] = i;
    for (uint32_t i = 1; i < cols; ++i) {
        const int o = order[i];
        const double v = A[o * PCA_B + o];
        uint32_t at = i;
        while (at > 0 && A[order[at - 1] * PCA_B + order[at - 1]] < v) { order[at] = order[at - 1]; --at; }
        order[at] = o;
    }
}

// ---- the rules of the contract
PCA_FN double pca_trace(uint64_t sum_h, uint32_t m) { return (double)sum_h / (double)m; }
PCA_FN bool pca_is_zero(double theta, double tol, double trace) { return !(theta > tol * trace); }
// theta descending: the pairs reported non-zero are a prefix of the first k
PCA_FN uint32_t pca_rank(const double *theta, uint32_t k, uint32_t cols, double tol, double trace) {
    uint32_t r = 0;
    while (r < k && r < cols && !pca_is_zero(theta[r], tol, trace)) ++r;
    return r;
}
PCA_FN bool pca_converged(const double *resid, const double *theta, uint32_t rank, double tol) {
    if (rank == 0) return false;  // trace > 0 here: a block that sees nothing yet has not converged
    for (uint32_t j = 0; j < rank; ++j)
        if (!(resid[j] <= tol * theta[0])) return false;
    return true;
}
// sign: the component of largest magnitude is positive, the lowest index on exact ties -> its index
PCA_FN uint32_t pca_sign_pivot(const double *v, uint32_t m) {
    uint32_t at = 0;
    for (uint32_t i = 1; i < m; ++i)
        if (fabs(v[i]) > fabs(v[at])) at = i;
    return at;
}
// lostruct's distance of two windows from their k eigenvalues and the k x k dot products v_j . v'_l (dots[j * k + l])
PCA_FN double pca_dist2(uint32_t k, const double *la, const double *lb, const double *dots) {
    double sa = 0.0, sb = 0.0;
    for (uint32_t j = 0; j < k; ++j) { sa += la[j]; sb += lb[j]; }
    if (!(sa > 0.0) || !(sb > 0.0)) return __builtin_nan("");
    double aa = 0.0, bb = 0.0, ab = 0.0;
    for (uint32_t j = 0; j < k; ++j) {
        const double a = la[j] / sa, b = lb[j] / sb;
        aa += a * a; bb += b * b;
    }
    // the terms (j, l) and (l, j) are added to each other first: swapping the two windows then swaps two addends and nothing
    // else, so d2(w, w') and d2(w', w) are the same bits whichever window comes first in the caller's list
    for (uint32_t j = 0; j < k; ++j)
        for (uint32_t l = j; l < k; ++l) {
            const double t = (la[j] / sa) * (lb[l] / sb) * (dots[j * k + l] * dots[j * k + l]);
            const double u = (la[l] / sa) * (lb[j] / sb) * (dots[l * k + j] * dots[l * k + j]);
            ab += l == j ? t : t + u;
        }
    const double d = (aa + bb) - 2.0 * ab;
    return d > 0.0 ? d : 0.0;
}

// ---- the whole iteration with plain loops, on the host: what pca.hip does with a workgroup.  H: m x m symmetric distances.
struct PcaSerialResult {
    uint32_t rank = 0, iterations = 0, flags = 0;
    uint64_t sum_h = 0;
    double lambda[PCA_MAX_K], resid[PCA_MAX_K];
    std::vector<double> vectors;  // k x m
};
inline void pca_jacobi_serial(double *A /* in: G, out: diagonalised */, double *Q /* out */) {
    double B2[PCA_B * PCA_B], Q2[PCA_B * PCA_B], cs[PCA_B], ts[PCA_B];
    for (int e = 0; e < PCA_B * PCA_B; ++e) Q[e] = (e / PCA_B == e % PCA_B) ? 1.0 : 0.0;
    const double thr = pca_jacobi_threshold(A);
    for (int sweep = 0; sweep < PCA_MAX_SWEEPS; ++sweep) {
        bool any = false;
        for (int i = 0; i < PCA_B; ++i)
            for (int j = i + 1; j < PCA_B; ++j) any = any || fabs(A[i * PCA_B + j]) > thr;
        if (!any) break;
        for (int round = 0; round < 15; ++round) {
            for (int x = 0; x < PCA_B; ++x) pca_jacobi_round_angles(A, thr, round, x, cs, ts);
            for (int e = 0; e < PCA_B * PCA_B; ++e) {
                B2[e] = pca_jacobi_elem(A, cs, ts, round, e / PCA_B, e % PCA_B);
                Q2[e] = pca_jacobi_qelem(Q, cs, ts, round, e / PCA_B, e % PCA_B);
            }
            for (int e = 0; e < PCA_B * PCA_B; ++e) { A[e] = B2[e]; Q[e] = Q2[e]; }
        }
    }
}
inline void pca_orthonormalise_serial(std::vector<double> &Z /* m x 16, row-major */, uint32_t m) {
    auto row = [&](uint32_t r) -> double(&)[PCA_B] { return *reinterpret_cast<double(*)[PCA_B]>(&Z[(size_t)r * PCA_B]); };
    double mean[PCA_B];
    for (int c = 0; c < PCA_B; ++c) {
        double s = 0.0;
        for (uint32_t r = 0; r < m; ++r) s += Z[(size_t)r * PCA_B + c];
        mean[c] = pca_mean(s, m);
    }
    for (uint32_t r = 0; r < m; ++r) pca_centre_row(row(r), mean);
    for (int j = 0; j < PCA_B; ++j) {
        double n0 = 0.0;
        for (int pass = 0; pass < 2; ++pass) {
            double p[PCA_B] = {0};
            for (uint32_t r = 0; r < m; ++r) pca_gs_partials(row(r), j, p);
            if (pass == 0) n0 = p[j];
            for (uint32_t r = 0; r < m; ++r) pca_gs_subtract(row(r), j, p);
        }
        double n2 = 0.0;
        for (uint32_t r = 0; r < m; ++r) n2 += pca_sq(Z[(size_t)r * PCA_B + j]);
        const double s = pca_gs_scale(n0, n2);
        for (uint32_t r = 0; r < m; ++r) Z[(size_t)r * PCA_B + j] *= s;
    }
}
inline PcaSerialResult pca_solve_serial(const uint32_t *H, uint32_t m, uint32_t k, double tol, uint32_t max_iter) {
    PcaSerialResult R;
    const double nan = __builtin_nan("");
    for (uint32_t j = 0; j < PCA_MAX_K; ++j) { R.lambda[j] = j < k ? 0.0 : nan; R.resid[j] = nan; }
    R.vectors.assign((size_t)k * m, 0.0);
    for (uint32_t i = 0; i < m; ++i)
        for (uint32_t j = i + 1; j < m; ++j) R.sum_h += H[(size_t)i * m + j];
    if (R.sum_h == 0) return R;
    const uint32_t cols = pca_block_cols(m);
    const double trace = pca_trace(R.sum_h, m);
    auto rowof = [](std::vector<double> &M, uint32_t r) -> double(&)[PCA_B] { return *reinterpret_cast<double(*)[PCA_B]>(&M[(size_t)r * PCA_B]); };
    std::vector<double> V((size_t)m * PCA_B), Z((size_t)m * PCA_B), X((size_t)m * PCA_B);
    for (uint32_t r = 0; r < m; ++r)
        for (int c = 0; c < PCA_B; ++c) V[(size_t)r * PCA_B + c] = pca_start(r, (uint32_t)c, cols);
    pca_orthonormalise_serial(V, m);
    double G[PCA_B * PCA_B], Q[PCA_B * PCA_B], Qs[PCA_B * PCA_B], theta[PCA_B], resid[PCA_B];
    int order[PCA_B];
    for (;;) {
        ++R.iterations;
        double sum[PCA_B] = {0}, mean[PCA_B];
        for (uint32_t r = 0; r < m; ++r) {
            double(&y)[PCA_B] = rowof(Z, r);
            for (int c = 0; c < PCA_B; ++c) y[c] = 0.0;
            for (uint32_t j = 0; j < m; ++j) pca_hv_add(y, (double)H[(size_t)j * m + r], &V[(size_t)j * PCA_B], 1);
            for (int c = 0; c < PCA_B; ++c) sum[c] += y[c];
        }
        for (int c = 0; c < PCA_B; ++c) mean[c] = pca_mean(sum[c], m);
        for (uint32_t r = 0; r < m; ++r) pca_bv_row(rowof(Z, r), mean);
        for (int i = 0; i < PCA_B; ++i) {
            double p[PCA_B] = {0};
            for (uint32_t r = 0; r < m; ++r) pca_dot_partials(V[(size_t)r * PCA_B + i], rowof(Z, r), p);
            for (int c = i; c < PCA_B; ++c) G[i * PCA_B + c] = G[c * PCA_B + i] = p[c];
        }
        pca_jacobi_serial(G, Q);
        pca_sort_desc(G, cols, order);
        for (int c = 0; c < PCA_B; ++c) {
            theta[c] = G[order[c] * PCA_B + order[c]];
            for (int d = 0; d < PCA_B; ++d) Qs[d * PCA_B + c] = Q[d * PCA_B + order[c]];
        }
        double p[PCA_B] = {0};
        for (uint32_t r = 0; r < m; ++r) {
            double zq[PCA_B];
            pca_rotate_row(rowof(Z, r), Qs, zq);
            pca_rotate_row(rowof(V, r), Qs, rowof(X, r));
            pca_resid_partials(zq, rowof(X, r), theta, p);
            for (int c = 0; c < PCA_B; ++c) Z[(size_t)r * PCA_B + c] = zq[c];
        }
        for (int c = 0; c < PCA_B; ++c) resid[c] = sqrt(p[c]);
        R.rank = pca_rank(theta, k, cols, tol, trace);
        const bool done = pca_converged(resid, theta, R.rank, tol);
        if (done || R.iterations >= max_iter) {
            R.flags = done ? 0u : PCA_FLAG_UNCONVERGED;
            break;
        }
        pca_orthonormalise_serial(Z, m);
        V = Z;
    }
    for (uint32_t j = 0; j < R.rank; ++j) {
        double *v = &R.vectors[(size_t)j * m];
        double s = 0.0, n = 0.0;
        for (uint32_t r = 0; r < m; ++r) s += X[(size_t)r * PCA_B + j];
        const double mean = pca_mean(s, m);
        for (uint32_t r = 0; r < m; ++r) { v[r] = X[(size_t)r * PCA_B + j] - mean; n += v[r] * v[r]; }
        const double scale = 1.0 / sqrt(n);
        for (uint32_t r = 0; r < m; ++r) v[r] *= scale;
        if (v[pca_sign_pivot(v, m)] < 0.0)
            for (uint32_t r = 0; r < m; ++r) v[r] = -v[r];
        R.lambda[j] = theta[j];
        R.resid[j] = resid[j];
    }
    return R;
}

}  // namespace impop
