// ldband_math.h — the arithmetic of impop_ldband_scan that is not a popcount (plain C++, no HIP types: tests/fuzz/ldband_math.cc
// compiles it on the host under the sanitizers; ldband.hip's pair and prune kernels run the same functions on the device).
//   ldband_fx       r2 of a site pair as a fixed-point integer: one IEEE division of exact values, an exact scaling by 2^30, an
//                   exact truncation, so 0 <= fx <= 2^30 and every sum of them is an integer sum.
//   ldband_strong   r2 > thr_num / thr_den without a division: num^2 thr_den > thr_num den in uint64 (num^2, den < 2^44 for
//                   n <= 4096; thr_num <= thr_den <= 65535: both products < 2^60).
//   ldband_bin      the decay bin of a coordinate distance.
//   kept window     the greedy pruning rule as a sliding register K of band_sites bits in 1..16 words of 64: bit o-1 = kept_{j-o}.
//                   kept_j = no word of (strongmask_j & K) is set; then K = (K << 1) | kept_j.  ldband_word_hit and
//                   ldband_word_shift are the rule for one word, so that the prune kernel can hold word w in lane w and pass the
//                   carry between lanes; ldband_kept_step is the same rule over an array of words.
#pragma once
#include <stdint.h>

#include "dip_runs.h"  // DIP_HD

#define LDBAND_FN DIP_HD inline __attribute__((always_inline))

namespace impop {

constexpr uint32_t LDBAND_MAX_N = 4096;     // IMPOP_LDBAND_MAX_N
constexpr uint32_t LDBAND_MAX_BAND = 1024;  // IMPOP_LDBAND_MAX_BAND
constexpr uint32_t LDBAND_MAX_BINS = 4096;  // IMPOP_LDBAND_MAX_BINS
constexpr uint32_t LDBAND_FX_ONE = 1u << 30;  // IMPOP_LDBAND_FX_ONE
constexpr uint32_t LDBAND_MAX_WORDS = LDBAND_MAX_BAND / 64;

LDBAND_FN uint32_t ldband_words(uint32_t band_sites) { return (band_sites + 63u) >> 6; }

// num = n n11 - c_s c_t, den = c_s (n - c_s) c_t (n - c_t) > 0
LDBAND_FN uint64_t ldband_fx(int64_t num, int64_t den) {
    const double r2 = (double)(num * num) / (double)den;
    return (uint64_t)(r2 * 1073741824.0);
}

LDBAND_FN bool ldband_perfect(int64_t num, int64_t den) { return num * num == den; }

LDBAND_FN bool ldband_strong(int64_t num, int64_t den, uint32_t thr_num, uint32_t thr_den) {
    return (uint64_t)(num * num) * (uint64_t)thr_den > (uint64_t)thr_num * (uint64_t)den;
}

LDBAND_FN uint32_t ldband_bin(uint64_t d, uint64_t bin_width, uint32_t n_bins) {
    const uint64_t b = d / bin_width;
    return b < (uint64_t)(n_bins - 1u) ? (uint32_t)b : n_bins - 1u;
}

// one word of the kept window: does a kept site stand where the strong mask has a bit; the word after the step, carry_in = the
// bit that enters at the bottom (kept_j for word 0, the top bit of the word below for the others)
LDBAND_FN bool ldband_word_hit(uint64_t k_word, uint64_t strong_word) { return (k_word & strong_word) != 0ull; }
LDBAND_FN uint64_t ldband_word_carry(uint64_t k_word) { return k_word >> 63; }
LDBAND_FN uint64_t ldband_word_shift(uint64_t k_word, uint64_t carry_in) { return (k_word << 1) | carry_in; }

// site j of a window, called for j = 0, 1, ..: K and strong hold `words` words, K all zero before site 0 -> kept_j
LDBAND_FN bool ldband_kept_step(uint64_t *K, const uint64_t *strong, uint32_t words) {
    bool hit = false;
    for (uint32_t w = 0; w < words; ++w) hit = hit || ldband_word_hit(K[w], strong[w]);
    uint64_t carry = hit ? 0ull : 1ull;
    for (uint32_t w = 0; w < words; ++w) {
        const uint64_t up = ldband_word_carry(K[w]);
        K[w] = ldband_word_shift(K[w], carry);
        carry = up;
    }
    return !hit;
}

}  // namespace impop
