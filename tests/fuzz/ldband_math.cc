// ldband_math.cc — stand-alone driver for csrc/ldband_math.h (no HIP): builds with a host compiler under ASan + UBSan.
//   ldband_math <seed> <rounds>
// Every round draws a band from {1, 63, 64, 65, 300, 1024} (each at least once), a number of sites q (0, 1, 2 in the first rounds,
// then random up to a few bands) and a random symmetric `strong` relation inside the band, packs strongmask_j as the pair kernel
// does (bit o-1 of word (o-1)/64 = strong(j-o, j)), and compares:
//   kept       ldband_kept_step over 1..16 words, and the same rule driven word by word through ldband_word_hit / _carry / _shift as
//              the prune kernel drives it across lanes, against the definition: kept_j = no kept i < j in the band is strong with j;
//   strong     ldband_strong against unsigned __int128 products, on random values and at the n = 4096 extremes
//              (num^2 = den = 2^44, thresholds 0/1, 1/1, 65535/65535, 65534/65535, 1/65535);
//   fx, bin    ldband_fx in 0..2^30 with fx == 2^30 iff perfect, monotone in num^2; ldband_bin against its definition.
// Prints "ok <rounds>" or the first difference.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "ldband_math.h"

using namespace impop;

static const uint32_t BANDS[6] = {1, 63, 64, 65, 300, 1024};

static bool strong128(int64_t num, int64_t den, uint32_t tn, uint32_t td) {
    const unsigned __int128 a = (unsigned __int128)(uint64_t)(num * num) * td, b = (unsigned __int128)tn * (uint64_t)den;
    return a > b;
}

static int check_strong(std::mt19937_64 &rng) {
    const int64_t top = (int64_t)1 << 22;  // |num| <= n^2 / 4, den <= (n^2 / 4)^2 at n = 4096
    const uint32_t thr[5][2] = {{0, 1}, {1, 1}, {65535, 65535}, {65534, 65535}, {1, 65535}};
    const int64_t nums[5] = {0, 1, -1, top, -top};
    const int64_t dens[4] = {1, 4095, top * top - 1, top * top};
    for (const auto &t : thr)
        for (int64_t num : nums)
            for (int64_t den : dens) {
                if (num * num > den) continue;  // r2 <= 1
                if (ldband_strong(num, den, t[0], t[1]) != strong128(num, den, t[0], t[1])) {
                    printf("strong: num %lld den %lld thr %u/%u\n", (long long)num, (long long)den, t[0], t[1]);
                    return 1;
                }
                if (t[0] == t[1] && ldband_strong(num, den, t[0], t[1])) {
                    printf("strong: r2 <= 1 exceeds a threshold of 1 (num %lld den %lld)\n", (long long)num, (long long)den);
                    return 1;
                }
            }
    for (int i = 0; i < 2000; ++i) {
        const int64_t den = 1 + (int64_t)(rng() % (uint64_t)(top * top));
        int64_t num = (int64_t)(rng() % (uint64_t)(top + 1));
        while (num * num > den) num /= 2;
        if (rng() & 1) num = -num;
        const uint32_t td = 1 + (uint32_t)(rng() % 65535), tn = (uint32_t)(rng() % (td + 1));
        if (ldband_strong(num, den, tn, td) != strong128(num, den, tn, td)) {
            printf("strong: num %lld den %lld thr %u/%u\n", (long long)num, (long long)den, tn, td);
            return 1;
        }
        const uint64_t fx = ldband_fx(num, den);
        if (fx > LDBAND_FX_ONE || (fx == LDBAND_FX_ONE) != ldband_perfect(num, den) || ldband_fx(-num, den) != fx) {
            printf("fx: num %lld den %lld fx %llu\n", (long long)num, (long long)den, (unsigned long long)fx);
            return 1;
        }
        if (num && ldband_fx(num / 2, den) > fx) {
            printf("fx is not monotone: num %lld den %lld\n", (long long)num, (long long)den);
            return 1;
        }
        const uint64_t d = rng() % 100000, bw = 1 + rng() % 5000;
        const uint32_t nb = 1 + (uint32_t)(rng() % LDBAND_MAX_BINS);
        const uint64_t want = d / bw < nb - 1 ? d / bw : nb - 1;
        if (ldband_bin(d, bw, nb) != want) {
            printf("bin: d %llu width %llu bins %u\n", (unsigned long long)d, (unsigned long long)bw, nb);
            return 1;
        }
    }
    if (ldband_fx(0, 7) != 0 || ldband_fx(top, top * top) != LDBAND_FX_ONE || ldband_fx(2, 12) != 357913941ull) {
        printf("fx: fixed points\n");
        return 1;
    }
    return 0;
}

int main(int argc, char **argv) {
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int rounds = argc > 2 ? atoi(argv[2]) : 100;
    std::mt19937_64 rng(seed);
    if (check_strong(rng)) return 1;
    for (int round = 0; round < rounds; ++round) {
        const uint32_t band = BANDS[round % 6], words = ldband_words(band);
        if (words < 1 || words > LDBAND_MAX_WORDS || words != (band + 63) / 64) {
            printf("words of band %u: %u\n", band, words);
            return 1;
        }
        const uint32_t q = round < 18 ? (uint32_t)(round / 6) : (uint32_t)(rng() % (3 * band + 70));
        const uint32_t p_strong = (uint32_t)(rng() % 1000) < 300 ? (uint32_t)(rng() % 1000) : (uint32_t)(rng() % 40);  // per mille
        // strongmask_j, exactly words words per site (the sanitizer sees an access past them)
        std::vector<uint64_t> sm((size_t)q * words, 0ull);
        for (uint32_t j = 0; j < q; ++j)
            for (uint32_t o = 1; o <= band && o <= j; ++o)
                if (rng() % 1000 < p_strong) sm[(size_t)j * words + ((o - 1) >> 6)] |= 1ull << ((o - 1) & 63);
        // the definition
        std::vector<char> want(q, 0);
        for (uint32_t j = 0; j < q; ++j) {
            bool hit = false;
            for (uint32_t o = 1; o <= band && o <= j && !hit; ++o)
                hit = want[j - o] && ((sm[(size_t)j * words + ((o - 1) >> 6)] >> ((o - 1) & 63)) & 1ull);
            want[j] = !hit;
        }
        // the array form, and the word-by-word form of the prune kernel (lane w holds word w; the carry comes from the word below)
        std::vector<uint64_t> K(words, 0ull), L(words, 0ull);
        for (uint32_t j = 0; j < q; ++j) {
            const bool kept = ldband_kept_step(K.data(), sm.data() + (size_t)j * words, words);
            bool any = false;
            for (uint32_t w = 0; w < words; ++w) any = any || ldband_word_hit(L[w], sm[(size_t)j * words + w]);
            std::vector<uint64_t> carry(words);
            for (uint32_t w = 0; w < words; ++w) carry[w] = w ? ldband_word_carry(L[w - 1]) : (any ? 0ull : 1ull);
            for (uint32_t w = 0; w < words; ++w) L[w] = ldband_word_shift(L[w], carry[w]);
            if (kept != (bool)want[j] || !any != (bool)want[j] || K != L) {
                printf("round %d band %u q %u site %u: kept %d / %d / %d\n", round, band, q, j, (int)kept, (int)!any, (int)want[j]);
                return 1;
            }
        }
        if (q && !want[0]) {
            printf("round %d: the first site is not kept\n", round);
            return 1;
        }
    }
    printf("ok %d\n", rounds);
    return 0;
}
