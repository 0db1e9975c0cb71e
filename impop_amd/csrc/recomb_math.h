// recomb_math.h — the per-window arithmetic of impop_recomb_scan (plain C++, no HIP types: tests/fuzz/recomb_math.cc compiles it on
// the host under the sanitizers; recomb.hip's finish kernel runs the same functions on the device).
//
// Input, per used site j = 0..m-1 in position order (recomb.hip's pair kernel): left1_j = 1 + the nearest site left of j that is
// incompatible with it under the four-gamete test (0: none), n_left_j = how many sites left of j are, rep_j = the first site with
// j's bipartition of the members.  One pass over j, constant state:
//   rmin     Hudson & Kaplan 1985.  Of all incompatible pairs (i, j) the open interval (left1_j - 1, j) is the shortest that ends
//            at j, so the largest set of disjoint intervals is found among those: greedy by right end, `cut` the right end of the
//            last interval taken; intervals that share an end point are disjoint.
//   blocks   M_j = max_{k<=j} left1_k: sites M_j..j are the longest pairwise compatible run that ends at j.  The run that ends at
//            j - 1 is maximal iff M_j > M_{j-1}; the one that ends at m - 1 always is.
//   Wall 1999: B' = adjacent congruent pairs, A = the distinct partitions those pairs show (one bit per rep value in `seen`).
#pragma once
#include <stdint.h>

#include "dip_runs.h"  // DIP_HD

#define RECOMB_FN DIP_HD inline __attribute__((always_inline))

namespace impop {

constexpr uint32_t RECOMB_MAX_N = 4096;       // IMPOP_RECOMB_MAX_N
constexpr uint32_t RECOMB_MAX_SITES = 16384;  // IMPOP_RECOMB_MAX_SITES

struct RecombState {
    uint64_t n_incompatible;
    uint32_t cut, rmin;                 // the greedy's last right end; intervals taken
    uint32_t M;                         // the running maximum of left1
    uint32_t n_adjacent;                // incompatible adjacent pairs
    uint32_t n_blocks, longest, longest_first, longest_last;  // maximal runs; the longest one and its first / last site
    uint32_t n_congruent_adjacent, n_congruent_partitions, n_partitions;
    uint32_t n_positive;                // sites with left1 > 0: rmin can never exceed it
    uint32_t prev_rep;
};

RECOMB_FN uint32_t recomb_seen_words(uint32_t m) { return (m + 31u) >> 5; }  // dwords of `seen`, zeroed by the caller

RECOMB_FN RecombState recomb_start() { return RecombState{0ull, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}; }

// site j, called for j = 0, 1, ..; true where the greedy takes the interval (left1 - 1, j)
RECOMB_FN bool recomb_step(RecombState &s, uint32_t j, uint32_t left1, uint32_t n_left, uint32_t rep, uint32_t *seen) {
    s.n_incompatible += n_left;
    s.n_positive += left1 != 0u;
    s.n_adjacent += j >= 1u && left1 == j;
    const bool taken = left1 >= 1u && left1 - 1u >= s.cut;
    if (taken) {
        ++s.rmin;
        s.cut = j;
    }
    if (left1 > s.M) {
        s.n_blocks += j >= 1u;  // the run that ends at j - 1 cannot be extended
        s.M = left1;
    }
    const uint32_t len = j - s.M + 1u;
    if (len > s.longest) {
        s.longest = len;
        s.longest_first = s.M;
        s.longest_last = j;
    }
    s.n_partitions += rep == j;
    if (j >= 1u && rep == s.prev_rep) {
        ++s.n_congruent_adjacent;
        const uint32_t bit = 1u << (rep & 31u);
        if (!(seen[rep >> 5] & bit)) {
            seen[rep >> 5] |= bit;
            ++s.n_congruent_partitions;
        }
    }
    s.prev_rep = rep;
    return taken;
}

RECOMB_FN void recomb_end(RecombState &s, uint32_t m) { s.n_blocks += m > 0u; }

// the whole window as plain loops: seen holds recomb_seen_words(m) dwords
inline RecombState recomb_solve_serial(const uint32_t *left1, const uint32_t *n_left, const uint32_t *rep, uint32_t m, uint32_t *seen) {
    for (uint32_t i = 0; i < recomb_seen_words(m); ++i) seen[i] = 0u;
    RecombState s = recomb_start();
    for (uint32_t j = 0; j < m; ++j) recomb_step(s, j, left1[j], n_left[j], rep[j], seen);
    recomb_end(s, m);
    return s;
}

}  // namespace impop
