// Stand-alone driver for csrc/kin_math.h (no HIP): random small genotype sets.  The joint table derived from the popcount Gram
// entries of the planes H = h1 ^ h2 and A = h1 & h2 must equal direct counting of the genotype pairs; the threshold test must equal
// an exact rational comparison in 128-bit integers, m = 0 and the ends num = 0 / num = den included; entries that cannot be one
// window's popcounts must be refused; the pair index must walk the order (0,1),(0,2),..,(1,2),...
// Build with -fsanitize=address,undefined.   usage: kin_math <seed> <iterations>
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "kin_math.h"

using namespace impop;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            printf("FAILED %s (line %d, iteration %d)\n", #cond, __LINE__, it); \
            return 1;                                                        \
        }                                                                    \
    } while (0)

static int64_t popc_and(const std::vector<uint64_t> &a, const std::vector<uint64_t> &b) {
    int64_t c = 0;
    for (size_t k = 0; k < a.size(); ++k) c += __builtin_popcountll(a[k] & b[k]);
    return c;
}

int main(int argc, char **argv) {
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int iters = argc > 2 ? atoi(argv[2]) : 1000;
    std::mt19937_64 rng(seed);
    auto below = [&](uint64_t n) { return (uint64_t)(rng() % n); };
    int it = 0;
    for (it = 0; it < iters; ++it) {
        const uint32_t N = 2 + (uint32_t)below(6), W = (uint32_t)below(200), words = (W + 63) / 64 + 1;
        // haplotypes with a random density, so that het = 0 and alt = 0 both occur
        const uint32_t dens = (uint32_t)below(5);
        std::vector<std::vector<uint8_t>> hap(2 * N, std::vector<uint8_t>(W));
        for (auto &h : hap)
            for (auto &b : h) b = dens == 0 ? 0 : dens == 4 ? 1 : (below(4) < dens ? 1 : 0);
        if (below(3) == 0) hap[1] = hap[0];  // a homozygous individual
        if (below(3) == 0) { hap[2] = hap[0]; hap[3] = hap[1]; }  // a duplicate
        std::vector<std::vector<uint64_t>> H(N, std::vector<uint64_t>(words, 0)), A(N, std::vector<uint64_t>(words, 0));
        for (uint32_t i = 0; i < N; ++i)
            for (uint32_t s = 0; s < W; ++s) {
                const uint8_t a = hap[2 * i][s], b = hap[2 * i + 1][s];
                if (a ^ b) H[i][s >> 6] |= 1ull << (s & 63);
                if (a & b) A[i][s >> 6] |= 1ull << (s & 63);
            }
        uint64_t expect_index = 0;
        for (uint32_t i = 0; i < N; ++i)
            for (uint32_t j = i + 1; j < N; ++j, ++expect_index) {
                CHECK(kin_pair_index(N, i, j) == expect_index);
                int64_t direct[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
                for (uint32_t s = 0; s < W; ++s) direct[3 * (hap[2 * i][s] + hap[2 * i + 1][s]) + hap[2 * j][s] + hap[2 * j + 1][s]] += 1;
                const int64_t het_i = popc_and(H[i], H[i]), alt_i = popc_and(A[i], A[i]), het_j = popc_and(H[j], H[j]), alt_j = popc_and(A[j], A[j]);
                const int64_t HH = popc_and(H[i], H[j]), HA = popc_and(H[i], A[j]), AH = popc_and(A[i], H[j]), AA = popc_and(A[i], A[j]);
                KinTable k;
                CHECK(kin_table(W, het_i, alt_i, het_j, alt_j, HH, HA, AH, AA, k));
                for (int c = 0; c < 9; ++c) CHECK(k.t[c] == direct[c]);
                CHECK(kin_het_het(k) == direct[4] && kin_ibs0(k) == direct[2] + direct[6] && kin_ibs2(k) == direct[0] + direct[4] + direct[8]);
                // a compacted window: c dropped all-ones sites count in alt and AA alone
                const int64_t c = (int64_t)below(50);
                KinTable kc;
                CHECK(kin_table(W + c, het_i, alt_i + c, het_j, alt_j + c, HH, HA, AH, AA + c, kc));
                for (int q = 0; q < 9; ++q) CHECK(kc.t[q] == direct[q] + (q == 8 ? c : 0));
                // entries that are no window's popcounts
                KinTable bad;
                CHECK(!kin_table(W, het_i, alt_i, het_j, alt_j, HH + het_i + 1, HA, AH, AA, bad));
                CHECK(!kin_table((int64_t)W - direct[0] - 1, het_i, alt_i, het_j, alt_j, HH, HA, AH, AA, bad));
                // the threshold against an exact rational comparison
                for (int rep = 0; rep < 6; ++rep) {
                    const int64_t den = rep == 0 ? 1 : rep == 1 ? (1 << 20) : 1 + (int64_t)below(1 << 20);
                    const int64_t num = rep == 2 ? 0 : rep == 3 ? den : (int64_t)below((uint64_t)den + 1);
                    const int64_t m = het_i < het_j ? het_i : het_j, hh = kin_het_het(k), i0 = kin_ibs0(k);
                    bool want = false;
                    if (m > 0) {  // (2 (hh - 2 i0) + 2 m - a - b) / (4 m) >= num / den
                        const __int128 lhs = (__int128)den * (2 * (hh - 2 * i0) + 2 * m - het_i - het_j), rhs = (__int128)4 * m * num;
                        want = lhs >= rhs;
                    }
                    CHECK(kin_related(het_i, het_j, hh, i0, num, den) == want);
                    if (m == 0) CHECK(!kin_related(het_i, het_j, hh, i0, 0, den));
                }
            }
    }
    // the widest admitted operands stay inside int64: W = 2^31 - 1, den = 2^20
    {
        const int64_t W = 0x7FFFFFFFll, den = 1 << 20;
        CHECK(kin_related(W, W, W, 0, den, den) == false);       // kinship 0.5 < 1
        CHECK(kin_related(W, W, W, 0, den / 2, den) == true);    // kinship 0.5 >= 0.5
        CHECK(kin_related(W, W, 0, W, 0, den) == false);         // the most negative numerator
        CHECK(kin_related(1, W, 0, 0, 0, den) == false && kin_related(1, 1, 1, 0, den / 2, den) == true);
    }
    printf("ok %d\n", iters);
    return 0;
}
