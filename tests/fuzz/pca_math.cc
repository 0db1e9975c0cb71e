// Stand-alone driver for csrc/pca_math.h (no HIP): the whole block iteration (pca_solve_serial) on the double-centred distance
// matrices of random small 0/1 matrices, checked against a brute-force cyclic Jacobi of the full matrix B built from the exact
// integers 2 m^2 B; the zero rule at its boundary; the sign rule on ties; the window distance against an explicit Frobenius norm.
// Build with -fsanitize=address,undefined.   usage: pca_math <seed> <iterations>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <vector>

#include "pca_math.h"

using namespace impop;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            printf("FAILED %s (line %d, iteration %d)\n", #cond, __LINE__, it); \
            return 1;                                                        \
        }                                                                    \
    } while (0)

// eigenvalues (descending) of a symmetric n x n matrix by classical cyclic Jacobi, row by row: nothing shared with the header
static std::vector<double> brute_eigenvalues(std::vector<double> A, int n) {
    for (int sweep = 0; sweep < 100; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < n; ++p)
            for (int q = p + 1; q < n; ++q) off += A[p * n + q] * A[p * n + q];
        if (off == 0.0) break;
        for (int p = 0; p < n; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = A[p * n + q];
                if (apq == 0.0) continue;
                const double th = (A[q * n + q] - A[p * n + p]) / (2.0 * apq);
                const double t = (th >= 0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0)), c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < n; ++k) {
                    const double akp = A[k * n + p], akq = A[k * n + q];
                    A[k * n + p] = c * akp - s * akq; A[k * n + q] = s * akp + c * akq;
                }
                for (int k = 0; k < n; ++k) {
                    const double apk = A[p * n + k], aqk = A[q * n + k];
                    A[p * n + k] = c * apk - s * aqk; A[q * n + k] = s * apk + c * aqk;
                }
            }
    }
    std::vector<double> ev(n);
    for (int i = 0; i < n; ++i) ev[i] = A[i * n + i];
    std::sort(ev.begin(), ev.end(), [](double a, double b) { return a > b; });
    return ev;
}

int main(int argc, char **argv) {
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int iters = argc > 2 ? atoi(argv[2]) : 100;
    std::mt19937_64 rng(seed);
    auto below = [&](uint32_t n) { return (uint32_t)(rng() % n); };
    const double eps = 2.220446049250313e-16, tol = 1e-10;
    int it = 0, solved = 0;

    // the round-robin order: every round pairs all 16 indexes, every pair meets exactly once in 15 rounds
    {
        int met[16][16] = {{0}};
        for (int r = 0; r < 15; ++r)
            for (int x = 0; x < 16; ++x) {
                const int y = pca_rr_partner(r, x);
                CHECK(y >= 0 && y < 16 && y != x && pca_rr_partner(r, y) == x);
                met[x][y] += 1;
            }
        for (int x = 0; x < 16; ++x)
            for (int y = 0; y < 16; ++y) CHECK(met[x][y] == (x != y));
    }
    // the zero rule at its boundary, the rank as a prefix, convergence
    {
        const double trace = 2.25, t = 1e-10;
        CHECK(pca_is_zero(t * trace, t, trace) && !pca_is_zero(nextafter(t * trace, 1.0), t, trace) && pca_is_zero(0.0, t, trace));
        CHECK(pca_is_zero(-1.0, t, trace) && pca_is_zero(__builtin_nan(""), t, trace));
        const double th[4] = {1.5, 0.5, t * trace, 0.25};
        CHECK(pca_rank(th, 4, 16, t, trace) == 2 && pca_rank(th, 1, 16, t, trace) == 1 && pca_rank(th, 4, 1, t, trace) == 1);
        const double r_ok[2] = {1.5e-10, 1e-12}, r_bad[2] = {1e-12, nextafter(1.5e-10, 1.0)};
        CHECK(pca_converged(r_ok, th, 2, t) && !pca_converged(r_bad, th, 2, t) && !pca_converged(r_ok, th, 0, t));
        CHECK(pca_trace(9, 4) == 2.25 && pca_block_cols(2) == 1 && pca_block_cols(17) == 16 && pca_block_cols(1024) == 16);
    }
    // the sign rule: the largest magnitude, the lowest index on exact ties
    {
        const double a[4] = {0.5, -0.5, 0.5, -0.5}, b[3] = {-0.25, 0.75, -0.75}, c[2] = {-0.7, 0.7};
        CHECK(pca_sign_pivot(a, 4) == 0 && pca_sign_pivot(b, 3) == 1 && pca_sign_pivot(c, 2) == 0);
    }

    for (it = 0; it < iters; ++it) {
        const uint32_t m = 2 + below(39), S = 1 + below(60), k = 1 + below(8);
        std::vector<uint8_t> X((size_t)m * S);
        for (auto &x : X) x = (uint8_t)(rng() & 1);
        for (uint32_t i = 1; i < m; ++i)  // copies and near-copies: repeated eigenvalues, low rank
            if (below(10) < 3) {
                memcpy(&X[(size_t)i * S], &X[(size_t)below(i) * S], S);
                if (below(2)) X[(size_t)i * S + below(S)] ^= 1;
            }
        if (it % 17 == 5)  // all identical: rank 0
            for (uint32_t i = 1; i < m; ++i) memcpy(&X[(size_t)i * S], &X[0], S);
        std::vector<uint32_t> H((size_t)m * m, 0);
        for (uint32_t i = 0; i < m; ++i)
            for (uint32_t j = 0; j < m; ++j)
                for (uint32_t s = 0; s < S; ++s) H[(size_t)i * m + j] += X[(size_t)i * S + s] != X[(size_t)j * S + s];
        // 2 m^2 B_ij = m (r_i + r_j) - m^2 H_ij - t, in integers
        std::vector<int64_t> r(m, 0);
        int64_t t = 0;
        for (uint32_t i = 0; i < m; ++i)
            for (uint32_t j = 0; j < m; ++j) { r[i] += H[(size_t)i * m + j]; t += H[(size_t)i * m + j]; }
        std::vector<double> B((size_t)m * m);
        for (uint32_t i = 0; i < m; ++i)
            for (uint32_t j = 0; j < m; ++j)
                B[(size_t)i * m + j] = (double)((int64_t)m * (r[i] + r[j]) - (int64_t)m * m * H[(size_t)i * m + j] - t) / (2.0 * m * m);
        const std::vector<double> ev = brute_eigenvalues(B, (int)m);
        const double trace = (double)t / 2.0 / m;
        const PcaSerialResult R = pca_solve_serial(H.data(), m, k, tol, 500);
        CHECK(R.sum_h == (uint64_t)t / 2);
        for (uint32_t j = k; j < PCA_MAX_K; ++j) CHECK(R.lambda[j] != R.lambda[j] && R.resid[j] != R.resid[j]);
        if (t == 0) {
            CHECK(R.rank == 0 && R.iterations == 0 && R.flags == 0);
            for (uint32_t j = 0; j < k; ++j) CHECK(R.lambda[j] == 0.0);
            continue;
        }
        // the guaranteed regime, from the exact spectrum: lambda_17 <= 0.9 lambda_j for the non-zero lambda_j, j <= k; and no
        // eigenvalue of the first k in the band where the zero rule could go either way
        bool regime = true;
        uint32_t want_rank = 0;
        for (uint32_t j = 0; j < k && j < m; ++j) {
            if (ev[j] > tol * trace) {
                if (want_rank == j) ++want_rank;
                if (m > 16 && !(ev[16] <= 0.9 * ev[j])) regime = false;
            }
            if (ev[j] > 1e-13 * trace && ev[j] < 1e-7 * trace) regime = false;
        }
        if (!regime) continue;
        ++solved;
        CHECK(R.flags == 0 && R.iterations >= 1 && R.iterations <= 500);
        CHECK(R.rank == want_rank);
        for (uint32_t j = 0; j < k; ++j) {
            const double *v = &R.vectors[(size_t)j * m];
            if (j >= R.rank) {
                CHECK(R.lambda[j] == 0.0 && R.resid[j] != R.resid[j]);
                for (uint32_t i = 0; i < m; ++i) CHECK(v[i] == 0.0);
                continue;
            }
            CHECK(fabs(R.lambda[j] - ev[j]) <= 2 * tol * ev[0]);
            CHECK(R.resid[j] <= tol * R.lambda[0]);
            double res = 0.0, one = 0.0;
            for (uint32_t i = 0; i < m; ++i) {
                double bv = 0.0;
                for (uint32_t l = 0; l < m; ++l) bv += B[(size_t)i * m + l] * v[l];
                res += (bv - R.lambda[j] * v[i]) * (bv - R.lambda[j] * v[i]);
                one += v[i];
            }
            CHECK(sqrt(res) <= 2 * tol * ev[0]);
            CHECK(fabs(one) <= 16 * m * eps);
            for (uint32_t l = 0; l <= j; ++l) {
                double d = 0.0;
                for (uint32_t i = 0; i < m; ++i) d += v[i] * R.vectors[(size_t)l * m + i];
                CHECK(fabs(d - (l == j ? 1.0 : 0.0)) <= 16 * m * eps);
            }
            const uint32_t at = pca_sign_pivot(v, m);
            CHECK(v[at] > 0.0);
            for (uint32_t i = 0; i < m; ++i) CHECK(fabs(v[i]) < fabs(v[at]) || (fabs(v[i]) == fabs(v[at]) && i >= at));
        }
        // the distance of this window to a copy of itself with the vectors negated, and to a second set of orthonormal vectors:
        // against || sum_j a_j v_j v_j^T - sum_l a'_l v'_l v'_l^T ||_F^2 written out
        if (R.rank >= 1) {
            std::vector<double> W2((size_t)k * m, 0.0), lam2(k, 0.0), dots((size_t)k * k), self((size_t)k * k);
            for (uint32_t j = 0; j < k; ++j) {  // a rotation of the pairs (j, j + 1) by a random angle keeps them orthonormal
                lam2[j] = R.lambda[j] * (1.0 + 0.25 * (double)below(4));
                for (uint32_t i = 0; i < m; ++i) W2[(size_t)j * m + i] = -R.vectors[(size_t)j * m + i];
            }
            if (R.rank >= 2) {
                const double ang = 0.1 + 0.01 * below(100), c = cos(ang), s = sin(ang);
                for (uint32_t i = 0; i < m; ++i) {
                    const double a = R.vectors[i], b = R.vectors[(size_t)m + i];
                    W2[i] = c * a - s * b; W2[(size_t)m + i] = s * a + c * b;
                }
            }
            for (uint32_t j = 0; j < k; ++j)
                for (uint32_t l = 0; l < k; ++l) {
                    double d = 0.0, e = 0.0;
                    for (uint32_t i = 0; i < m; ++i) {
                        d += R.vectors[(size_t)j * m + i] * W2[(size_t)l * m + i];
                        e += R.vectors[(size_t)j * m + i] * -R.vectors[(size_t)l * m + i];
                    }
                    dots[(size_t)j * k + l] = d; self[(size_t)j * k + l] = e;
                }
            const double d2 = pca_dist2(k, R.lambda, lam2.data(), dots.data());
            double sa = 0.0, sb = 0.0, fro = 0.0;
            for (uint32_t j = 0; j < k; ++j) { sa += R.lambda[j]; sb += lam2[j]; }
            for (uint32_t i = 0; i < m; ++i)
                for (uint32_t l = 0; l < m; ++l) {
                    double a = 0.0;
                    for (uint32_t j = 0; j < k; ++j)
                        a += R.lambda[j] / sa * R.vectors[(size_t)j * m + i] * R.vectors[(size_t)j * m + l] -
                             lam2[j] / sb * W2[(size_t)j * m + i] * W2[(size_t)j * m + l];
                    fro += a * a;
                }
            CHECK(fabs(d2 - fro) <= 64.0 * k * k * m * eps);
            CHECK(pca_dist2(k, R.lambda, R.lambda, self.data()) <= 4.0 * k * k * m * eps);  // sign flips change nothing
            const std::vector<double> zero(k, 0.0);
            const double dn = pca_dist2(k, R.lambda, zero.data(), dots.data());
            CHECK(dn != dn);
        }
    }
    it = -1;
    CHECK(iters < 20 || solved * 2 >= iters);  // the regime filter must leave most cases standing
    printf("ok %d\n", iters);
    return 0;
}
