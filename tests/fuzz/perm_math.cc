// Stand-alone driver for csrc/perm_math.h (no HIP).  Random small symmetric H: perm_window_serial against the definition restated
// here over SETS of positions (pairs inside a set, nearest-neighbour lists), the quadratic-form algebra (y = H z, r = H 1) against
// the direct sums, the generator's labellings (exactly m_a ones, none at or beyond m, a function of (seed, p, r) alone), and the
// 128-bit comparisons at the refusal bound W P^2 = 2^62 against a schoolbook product of 32-bit limbs.
// Build with -fsanitize=address,undefined.   usage: perm_math <seed> <iterations>  |  perm_math known
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#include "perm_math.h"

using namespace impop;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            printf("FAILED %s (line %d, iteration %d)\n", #cond, __LINE__, it); \
            return 1;                                                        \
        }                                                                    \
    } while (0)

// hi and lo of a * b from 32-bit limbs
static void mul_limbs(uint64_t a, uint64_t b, uint64_t *hi, uint64_t *lo) {
    const uint64_t a0 = a & 0xFFFFFFFFull, a1 = a >> 32, b0 = b & 0xFFFFFFFFull, b1 = b >> 32;
    const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const uint64_t mid = (p00 >> 32) + (p01 & 0xFFFFFFFFull) + (p10 & 0xFFFFFFFFull);
    *lo = (p00 & 0xFFFFFFFFull) | (mid << 32);
    *hi = p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
}
static bool le_limbs(uint64_t a, uint64_t b, uint64_t c, uint64_t d) {  // a b <= c d
    uint64_t h1, l1, h2, l2;
    mul_limbs(a, b, &h1, &l1);
    mul_limbs(c, d, &h2, &l2);
    return h1 < h2 || (h1 == h2 && l1 <= l2);
}

// the definition over sets: A = the ones of z, B = the zeros
static void by_sets(const std::vector<uint32_t> &H, uint32_t m, const uint64_t *z, uint64_t *wa, uint64_t *wb, uint64_t *nn) {
    std::vector<uint32_t> A, B;
    for (uint32_t i = 0; i < m; ++i) (perm_bit(z, i) ? A : B).push_back(i);
    *wa = *wb = *nn = 0;
    for (size_t x = 0; x < A.size(); ++x)
        for (size_t y = x + 1; y < A.size(); ++y) *wa += H[(size_t)A[x] * m + A[y]];
    for (size_t x = 0; x < B.size(); ++x)
        for (size_t y = x + 1; y < B.size(); ++y) *wb += H[(size_t)B[x] * m + B[y]];
    for (uint32_t i = 0; i < m; ++i) {
        uint32_t d = 0xFFFFFFFFu;
        for (uint32_t j = 0; j < m; ++j)
            if (j != i && H[(size_t)i * m + j] < d) d = H[(size_t)i * m + j];
        uint32_t tied = 0, same = 0;
        const std::vector<uint32_t> &own = perm_bit(z, i) ? A : B, &other = perm_bit(z, i) ? B : A;
        for (uint32_t j : own)
            if (j != i && H[(size_t)i * m + j] == d) { ++tied; ++same; }
        for (uint32_t j : other)
            if (H[(size_t)i * m + j] == d) ++tied;
        *nn += (uint64_t)same * (PERM_SCALE / tied);
    }
}

static int known() {
    // haplotypes 0000, 0001, 0111, 0001; panels {0,1} and {2,3}
    const uint32_t H[16] = {0, 1, 3, 1, 1, 0, 2, 0, 3, 2, 0, 2, 1, 0, 2, 0};
    const uint64_t z0 = 3, labels[6] = {3, 5, 9, 6, 10, 12};
    PermObs o;
    uint32_t st[4], ge[4];
    uint64_t null[18];
    perm_window_serial(H, 4, 2, &z0, labels, 6, &o, st, ge, null);
    printf("obs %llu %llu %llu %llu\n", (unsigned long long)o.wa, (unsigned long long)o.wb, (unsigned long long)o.nn, (unsigned long long)o.tot);
    printf("st %u/%u %u/%u %u/%u %u/%u\n", st[0] >> 16, st[0] & 0xFFFF, st[1] >> 16, st[1] & 0xFFFF, st[2] >> 16, st[2] & 0xFFFF, st[3] >> 16,
           st[3] & 0xFFFF);
    for (int r = 0; r < 6; ++r)
        printf("null %llu %llu %llu\n", (unsigned long long)null[3 * r], (unsigned long long)null[3 * r + 1], (unsigned long long)null[3 * r + 2]);
    printf("ge %u %u %u %u\n", ge[0], ge[1], ge[2], ge[3]);
    const PermDoubles d = perm_doubles(o, 2, 2);
    printf("doubles %.17g %.17g %.17g %.17g\n", d.fst, d.phi_st, d.dxy, perm_snn(st, 4));
    // the degenerate comparisons: ab(z) = 0 with x(z) > 0 is not counted, tot = 0 counts every labelling, tied = 17 floors
    const PermObs a{1, 2, 0, 9}, zero{0, 0, 0, 0};
    printf("degenerate %d %d %d %d %u\n", (int)perm_ge_fst(4, 5, a, 2, 2), (int)perm_ge_fst(0, 0, zero, 2, 2), (int)perm_ge_dxy(0, 0, zero),
           (int)perm_ge_phi(0, 0, zero, 2, 2), perm_nn_term(17));
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "known")) return known();
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int iters = argc > 2 ? atoi(argv[2]) : 300;
    std::mt19937_64 rng(seed);
    auto below = [&](uint64_t n) { return (uint64_t)(rng() % n); };
    int it = 0;
    for (it = 0; it < iters; ++it) {
        const uint32_t m = it % 7 == 0 ? 60 + (uint32_t)below(12) : 2 + (uint32_t)below(14), m_k = 1 + (uint32_t)below(m - 1), mw = (m + 63) / 64;
        const uint32_t range = it % 3 == 0 ? 2 : it % 3 == 1 ? 7 : 100000;  // many ties | some | none
        std::vector<uint32_t> H((size_t)m * m, 0);
        for (uint32_t i = 0; i < m; ++i)
            for (uint32_t j = i + 1; j < m; ++j) H[(size_t)i * m + j] = H[(size_t)j * m + i] = (uint32_t)below(range);
        const uint32_t n_perm = 1 + (uint32_t)below(9), pidx = (uint32_t)below(28);
        std::vector<uint64_t> labels((size_t)n_perm * mw), z0(mw, 0), again(mw);
        std::vector<uint32_t> a(m);
        for (uint32_t r = 0; r < n_perm; ++r) {
            perm_labelling(seed, pidx, r, m, m_k, a.data(), &labels[(size_t)r * mw]);
            uint32_t ones = 0;
            for (uint32_t w = 0; w < mw; ++w) ones += (uint32_t)__builtin_popcountll(labels[(size_t)r * mw + w]);
            CHECK(ones == m_k);
            CHECK((m & 63u) == 0 || (labels[(size_t)r * mw + mw - 1] >> (m & 63u)) == 0);
        }
        perm_labelling(seed, pidx, n_perm - 1, m, m_k, a.data(), again.data());  // alone: the same labelling
        CHECK(!memcmp(again.data(), &labels[(size_t)(n_perm - 1) * mw], mw * 8));
        for (uint32_t c = 0, i = 0; c < m_k; ++i)  // an observed labelling: a random m_k-subset
            if (below(m - i) < m_k - c) { z0[i >> 6] |= 1ull << (i & 63u); ++c; }
        PermObs o;
        std::vector<uint32_t> st(m);
        std::vector<uint64_t> null((size_t)n_perm * 3);
        uint32_t ge[4];
        perm_window_serial(H.data(), m, m_k, z0.data(), labels.data(), n_perm, &o, st.data(), ge, null.data());
        uint64_t wa, wb, nn, tot = 0;
        for (uint32_t i = 0; i < m; ++i)
            for (uint32_t j = 0; j < i; ++j) tot += H[(size_t)i * m + j];
        by_sets(H, m, z0.data(), &wa, &wb, &nn);
        CHECK(o.wa == wa && o.wb == wb && o.nn == nn && o.tot == tot);
        uint32_t want[4] = {0, 0, 0, 0};
        const uint64_t m_l = m - m_k, qk = perm_q(m_k), ql = perm_q(m_l);
        for (uint32_t r = 0; r < n_perm; ++r) {
            const uint64_t *z = &labels[(size_t)r * mw];
            by_sets(H, m, z, &wa, &wb, &nn);
            CHECK(null[3 * r] == wa && null[3 * r + 1] == wb && null[3 * r + 2] == nn);
            // the quadratic form: y = H z, r = H 1
            uint64_t zHz = 0, zr = 0, sum_r = 0;
            for (uint32_t i = 0; i < m; ++i) {
                uint64_t y = 0, ri = 0;
                for (uint32_t j = 0; j < m; ++j) { ri += H[(size_t)i * m + j]; if (perm_bit(z, j)) y += H[(size_t)i * m + j]; }
                sum_r += ri;
                if (perm_bit(z, i)) { zHz += y; zr += ri; }
            }
            uint64_t qa, qb;
            perm_wa_wb(zHz, zr, sum_r, &qa, &qb);
            CHECK(qa == wa && qb == wb && sum_r == 2 * tot);
            const uint64_t ab = tot - wa - wb, ab0 = tot - o.wa - o.wb;
            want[0] += le_limbs(wa * ql + wb * qk, ab0, o.wa * ql + o.wb * qk, ab) ? 1u : 0u;
            want[1] += wa * m_l + wb * m_k <= o.wa * m_l + o.wb * m_k ? 1u : 0u;
            want[2] += ab >= ab0 ? 1u : 0u;
            want[3] += nn >= o.nn ? 1u : 0u;
        }
        CHECK(ge[0] == want[0] && ge[1] == want[1] && ge[2] == want[2] && ge[3] == want[3]);
    }
    // the refusal bound: W P^2 = 2^62 is admitted, one more is not; at the bound x stays below 2^63 and the products are exact
    {
        const uint64_t P = 1ull << 15, W = 1ull << 32;  // (a bound on the arithmetic, not a shape the call accepts: W <= 2^31 there)
        CHECK(perm_fst_admitted(W, P) && !perm_fst_admitted(W + 1, P) && !perm_fst_admitted(W, P + 1));
        CHECK(perm_fst_admitted(0, 1ull << 40) && perm_fst_admitted(1, 1ull << 31) && !perm_fst_admitted(1, (1ull << 31) + 1));
        CHECK(!perm_fst_admitted(1ull << 63, 1ull << 63));
        const uint64_t m_k = 257, m_l = 257;  // q = 32896 > 2^15: use the admitted W for it
        const uint64_t q = perm_q(m_k), Wq = ((uint64_t)1 << 62) / (q * q);
        CHECK(perm_fst_admitted(Wq, q) && !perm_fst_admitted(Wq + 1, q));
        const uint64_t wa = Wq * q, wb = Wq * q, ab = Wq * m_k * m_l;  // every distance at its largest
        const PermObs o{wa, wb, 0, wa + wb + ab};
        const uint64_t x = wa * q + wb * q;
        CHECK(x < (1ull << 63) && x / q == wa + wb);
        for (uint64_t da = 0; da < 3; ++da) {
            const uint64_t za = wa - da, zb = wb - (2 - da);  // labellings next to the observed one
            const uint64_t zab = o.tot - za - zb;
            CHECK(perm_ge_fst(za, zb, o, m_k, m_l) == le_limbs(za * q + zb * q, ab, x, zab));
            CHECK(perm_ge_fst(za, zb, o, m_k, m_l));  // smaller within sums, larger ab: more differentiated
        }
        CHECK(perm_ge_fst(wa, wb, o, m_k, m_l) && perm_ge_phi(wa, wb, o, m_k, m_l) && perm_ge_dxy(wa, wb, o));
    }
    // the terms: every tied <= 16 divides SCALE; 17 floors
    for (uint32_t t = 1; t <= 16; ++t) CHECK(PERM_SCALE % t == 0 && (uint64_t)perm_nn_term(t) * t == PERM_SCALE);
    CHECK(PERM_SCALE == 720720ull * 4096ull && perm_nn_term(17) == 173651124u && PERM_SCALE % 17 != 0);
    printf("ok %d\n", iters);
    return 0;
}
