// recomb_math.cc — stand-alone driver for csrc/recomb_math.h (no HIP): builds with a host compiler under ASan + UBSan.
//   recomb_math <seed> <rounds>
// Every round draws random per-site arrays (left1_j <= j; rep_j = j or the rep of an earlier site), runs the header's one-pass
// scheme (recomb_solve_serial: what the finish kernel runs) and compares every counter with brute force:
//   rmin     the maximum number of pairwise disjoint open intervals (left1_j - 1, j) by dynamic programming over the right ends
//            (intervals that share an end point are disjoint);
//   blocks   all runs a..b with left1_k <= a for every k in a..b by an O(m^2) search, the maximal ones counted, the longest found
//            with ties to the smallest last site;
//   Wall     B', A and the partitions from their definitions, A through a plain boolean array.
// m = 0, 1 and 2 are drawn in every run.  Prints "ok <rounds>" or the first difference.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <random>
#include <vector>

#include "recomb_math.h"

using namespace impop;

struct Brute {
    uint64_t n_incompatible = 0;
    uint32_t rmin = 0, n_adjacent = 0, n_blocks = 0, longest = 0, first = 0, last = 0, b_prime = 0, a = 0, n_partitions = 0;
};

static Brute brute(const std::vector<uint32_t> &left1, const std::vector<uint32_t> &n_left, const std::vector<uint32_t> &rep) {
    const uint32_t m = (uint32_t)left1.size();
    Brute B;
    for (uint32_t j = 0; j < m; ++j) B.n_incompatible += n_left[j];
    for (uint32_t j = 1; j < m; ++j) B.n_adjacent += left1[j] == j;
    // best[p] = the most disjoint intervals with right end <= p
    std::vector<uint32_t> best(m + 1, 0);
    for (uint32_t p = 0; p < m; ++p) {
        uint32_t v = p ? best[p - 1] : 0;
        if (left1[p] >= 1) v = std::max(v, best[left1[p] - 1] + 1);  // the interval (left1 - 1, p) after everything that ends by left1 - 1
        best[p] = v;
    }
    B.rmin = m ? best[m - 1] : 0;
    // compatible runs
    auto ok = [&](uint32_t a, uint32_t b) {
        for (uint32_t k = a; k <= b; ++k)
            if (left1[k] > a) return false;
        return true;
    };
    for (uint32_t b = 0; b < m; ++b)
        for (uint32_t a = 0; a <= b; ++a) {
            if (!ok(a, b)) continue;
            const bool left_ext = a > 0 && ok(a - 1, b), right_ext = b + 1 < m && ok(a, b + 1);
            if (!left_ext && !right_ext) ++B.n_blocks;
            if (b - a + 1 > B.longest) {
                B.longest = b - a + 1;
                B.first = a;
                B.last = b;
            }
        }
    std::vector<char> in_pair(m, 0), seen(m, 0);
    for (uint32_t j = 1; j < m; ++j)
        if (rep[j] == rep[j - 1]) {
            ++B.b_prime;
            in_pair[j] = in_pair[j - 1] = 1;
        }
    for (uint32_t j = 0; j < m; ++j) {
        B.n_partitions += rep[j] == j;
        if (in_pair[j] && !seen[rep[j]]) {
            seen[rep[j]] = 1;
            ++B.a;
        }
    }
    return B;
}

int main(int argc, char **argv) {
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int rounds = argc > 2 ? atoi(argv[2]) : 100;
    std::mt19937_64 rng(seed);
    for (int round = 0; round < rounds; ++round) {
        const uint32_t m = round < 3 ? (uint32_t)round : (uint32_t)(rng() % 70);
        const uint32_t p_inc = (uint32_t)(rng() % 100), p_new = (uint32_t)(rng() % 100);
        std::vector<uint32_t> left1(m), n_left(m), rep(m);
        for (uint32_t j = 0; j < m; ++j) {
            left1[j] = j && rng() % 100 < p_inc ? 1 + (uint32_t)(rng() % j) : 0;
            n_left[j] = left1[j] ? 1 + (uint32_t)(rng() % left1[j]) : 0;
            rep[j] = j && rng() % 100 >= p_new ? rep[rng() % j] : j;
        }
        std::vector<uint32_t> seen(recomb_seen_words(m) + 1, 0xFFFFFFFFu);  // stale bits: the solver clears what it uses
        const RecombState s = recomb_solve_serial(left1.data(), n_left.data(), rep.data(), m, seen.data());
        const Brute B = brute(left1, n_left, rep);
        uint32_t positive = 0;
        for (uint32_t j = 0; j < m; ++j) positive += left1[j] != 0;
        const bool same = s.n_incompatible == B.n_incompatible && s.rmin == B.rmin && s.n_adjacent == B.n_adjacent && s.n_blocks == B.n_blocks &&
                          s.longest == B.longest && s.longest_first == B.first && s.longest_last == B.last &&
                          s.n_congruent_adjacent == B.b_prime && s.n_congruent_partitions == B.a && s.n_partitions == B.n_partitions &&
                          s.n_positive == positive && s.rmin <= positive;
        if (!same) {
            printf("round %d m %u: rmin %u/%u blocks %u/%u longest %u[%u..%u]/%u[%u..%u] B' %u/%u A %u/%u partitions %u/%u adjacent %u/%u\n", round,
                   m, s.rmin, B.rmin, s.n_blocks, B.n_blocks, s.longest, s.longest_first, s.longest_last, B.longest, B.first, B.last,
                   s.n_congruent_adjacent, B.b_prime, s.n_congruent_partitions, B.a, s.n_partitions, B.n_partitions, s.n_adjacent, B.n_adjacent);
            return 1;
        }
    }
    printf("ok %d\n", rounds);
    return 0;
}
