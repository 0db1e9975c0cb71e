// ihs_math.cc — stand-alone check of csrc/ihs_math.h (the arithmetic impop_ihs_scan shares between host and device) against a
// step-by-step model of its own.  Built with -fsanitize=address,undefined by tests/test_ihs_math_host.py.
//
//     ihs_math <seed> <iterations>   ->  "ok <iterations>"
//
// Per iteration: random rows made of a few founders with mutations, random coordinates, limits, cutoff, direction, and a random
// chunk [o0, o1) of the stepped ordinals.  The model counts, pair by pair from the rows, how many pairs of a class survive j
// steps from a core and integrates as the header's definitions say.  The code under test runs a serial PBWT from the chunk's
// warm-up start (divergences in steps, clipped at the start), takes the break weights from ihs_span_left / ihs_span_right with
// group maxima, finds the stop by bisection on ihs_cut_ok and sums ihs_break_term / ihs_alive_term — the walk kernel's
// arithmetic in the kernel's order.  Classes are by allele and by a random two-population labelling.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "ihs_math.h"

using namespace impop;

static uint64_t rng_state;
static uint64_t rnd() {
    rng_state += 0x9E3779B97F4A7C15ull;
    uint64_t x = rng_state;
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}
static uint64_t below(uint64_t n) { return rnd() % n; }

#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                  \
            fprintf(stderr, "\n");                         \
            exit(1);                                       \
        }                                                  \
    } while (0)

struct Result {
    uint64_t I2[2];
    uint32_t flags;
};

int main(int argc, char **argv) {
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int iters = argc > 2 ? atoi(argv[2]) : 100;
    rng_state = seed * 0x2545F4914F6CDD1Dull + 12345;
    for (int it = 0; it < iters; ++it) {
        // ---- a case: n rows over S stepped sites (every site polymorphic), ascending coordinates
        const uint32_t n = 2 + (uint32_t)below(it % 7 == 0 ? 90 : 24), nf = 1 + (uint32_t)below(4);
        const uint32_t S_raw = 1 + (uint32_t)below(70);
        std::vector<std::vector<uint8_t>> founders(nf, std::vector<uint8_t>(S_raw)), rows(n, std::vector<uint8_t>(S_raw));
        for (auto &f : founders)
            for (auto &b : f) b = (uint8_t)below(2);
        for (auto &r : rows) {
            uint32_t f = (uint32_t)below(nf);
            for (uint32_t s = 0; s < S_raw; ++s) {
                if (below(25) == 0) f = (uint32_t)below(nf);
                r[s] = founders[f][s] ^ (below(40) == 0 ? 1 : 0);
            }
        }
        std::vector<uint32_t> keep;
        for (uint32_t s = 0; s < S_raw; ++s) {
            uint32_t c = 0;
            for (auto &r : rows) c += r[s];
            if (c > 0 && c < n) keep.push_back(s);
        }
        const uint64_t S = keep.size();
        if (S == 0) continue;
        std::vector<uint64_t> posv(S);
        uint64_t p = below(1000);
        for (uint64_t x = 0; x < S; ++x) {
            p += 1 + (below(3) == 0 ? below(50) : 0);
            posv[x] = p;
        }
        auto bit = [&](uint32_t h, uint64_t x) { return rows[h][keep[x]]; };
        auto pos = [&](uint64_t i) { return posv[i]; };
        const uint64_t max_bp = below(3) == 0 ? 0 : 1 + below(80), max_sites = below(3) == 0 ? 0 : 1 + below(12);
        const uint32_t cutoff = below(4) == 0 ? (uint32_t)(below(2) * 1000) : (uint32_t)below(1001);
        const int dir = (int)below(2);
        const uint64_t o0 = below(S), o1 = o0 + 1 + below(S - o0);
        std::vector<uint8_t> lab(n);
        for (auto &l : lab) l = (uint8_t)below(2);

        // ---- lower bound and reach against linear scans
        for (int k = 0; k < 4; ++k) {
            const uint64_t v = below(p + 60);
            uint64_t lin = 0;
            while (lin < S && posv[lin] < v) ++lin;
            CHECK(ihs_lower_bound(pos, S, v) == lin, "lower_bound");
        }
        auto far_model = [&](int measure, uint64_t x, uint64_t limit) {
            uint64_t y = x;
            for (;;) {
                if (dir ? y + 1 >= S : y == 0) break;
                const uint64_t nx = dir ? y + 1 : y - 1;
                const uint64_t dist = measure ? (nx > x ? nx - x : x - nx) : (posv[nx] > posv[x] ? posv[nx] - posv[x] : posv[x] - posv[nx]);
                if (limit && dist > limit) break;
                y = nx;
            }
            return y;
        };
        uint64_t carried = 0;  // the reach of the last core visited, a few cores skipped in between as a walk does
        bool have = false;
        for (uint64_t k = 0; k < S; ++k) {
            const uint64_t x = dir ? S - 1 - k : k;
            if (have && below(3) == 0) continue;
            carried = have ? ihs_far_advance(dir, carried, x, S, max_bp, pos) : ihs_far(dir, 0, x, S, max_bp, pos);
            have = true;
            CHECK(carried == far_model(0, x, max_bp), "far_advance x=%llu", (unsigned long long)x);
        }
        for (uint64_t x = 0; x < S; ++x) {
            CHECK(ihs_far(dir, 0, x, S, max_bp, pos) == far_model(0, x, max_bp), "far bp x=%llu", (unsigned long long)x);
            CHECK(ihs_far(dir, 1, x, S, max_sites, pos) == far_model(1, x, max_sites), "far sites x=%llu", (unsigned long long)x);
        }
        const uint64_t ws = ihs_warm_start(dir, o0, o1, S, max_bp, max_sites, pos);
        {  // no stepped site of the chunk reaches beyond it, and it is a reach of the chunk's first
            for (uint64_t x = o0; x < o1; ++x)
                for (int m = 0; m < 2; ++m) {
                    const uint64_t f = far_model(m, x, m ? max_sites : max_bp);
                    CHECK(dir ? f <= ws : f >= ws, "warm start too near");
                }
            const uint64_t x = dir ? o1 - 1 : o0;
            CHECK(ws == far_model(0, x, max_bp) || ws == far_model(1, x, max_sites), "warm start is no reach");
        }

        // ---- chunks: a partition of the blocks, in order
        {
            const uint64_t n_blk = 1 + below(300);
            const IhsChunks c = ihs_chunks(n_blk, 1 + below(20000), 1 + below(1000000), below(2) ? below(100000) : 0, below(2) ? below(300) : 0,
                                           below(2) ? (uint32_t)(1 + below(40)) : 0, (uint32_t)below(300));
            uint64_t at = 0;
            CHECK(c.count() >= 1 && c.chunk_blocks >= 1, "chunks");
            for (uint64_t k = 0; k < c.count(); ++k) {
                CHECK(c.begin(k) == at && c.end(k) > at && c.end(k) <= n_blk, "chunk %llu", (unsigned long long)k);
                at = c.end(k);
            }
            CHECK(at == n_blk, "chunks do not cover");
        }

        // ---- the serial PBWT from the warm-up start; divergences in steps
        const uint32_t n_steps = (uint32_t)(dir ? ws - o0 + 1 : o1 - ws);
        std::vector<uint32_t> ord(n), dv(n, 0), ord2(n), dv2(n);
        for (uint32_t i = 0; i < n; ++i) ord[i] = i;
        auto ordinal = [&](uint32_t step) { return dir ? ws - step : ws + step; };
        // stable partition by key(member) with the carried maximum, as the kernel's (first of either side: sentinel)
        auto partition = [&](const std::vector<uint32_t> &so, const std::vector<uint32_t> &sd, std::vector<uint32_t> &dO,
                             std::vector<uint32_t> &dd, uint32_t sentinel, auto key) {
            uint32_t Z = 0;
            for (uint32_t i = 0; i < n; ++i) Z += key(so[i]) ? 0 : 1;
            uint32_t u = 0, v = Z, pmax = sentinel, qmax = sentinel;  // pmax: max of d since the last zero, qmax: since the last one
            for (uint32_t i = 0; i < n; ++i) {
                pmax = std::max(pmax, sd[i]);
                qmax = std::max(qmax, sd[i]);
                if (!key(so[i])) {
                    dO[u] = so[i];
                    dd[u++] = pmax;
                    pmax = 0;
                } else {
                    dO[v] = so[i];
                    dd[v++] = qmax;
                    qmax = 0;
                }
            }
            return Z;
        };
        for (uint32_t s = 0; s < n_steps; ++s) {
            const uint64_t x = ordinal(s);
            const uint32_t Z = partition(ord, dv, ord2, dv2, s + 1, [&](uint32_t h) { return bit(h, x); });
            ord.swap(ord2);
            dv.swap(dv2);
            const bool own = dir ? x < o1 : x >= o0;
            if (!own) continue;
            for (int K = 1; K <= 2; ++K) {
                std::vector<uint32_t> CO = ord, CD = dv;
                uint32_t split = Z;
                if (K == 2) {
                    std::vector<uint32_t> o3(n), d3(n);
                    split = partition(ord, dv, o3, d3, s + 1, [&](uint32_t h) { return lab[h]; });
                    CO = o3;
                    CD = d3;
                }
                std::vector<uint32_t> gmaxv((n + 31) / 32 + 1, 0);
                for (uint32_t i = 0; i < n; ++i) gmaxv[i >> 5] = std::max(gmaxv[i >> 5], CD[i]);
                auto dval = [&](uint32_t i) { return CD[i]; };
                auto gm = [&](uint32_t g) { return gmaxv[g]; };
                const uint64_t far[2] = {ihs_far(dir, 0, x, S, max_bp, pos), ihs_far(dir, 1, x, S, max_sites, pos)};
                uint32_t lb[2];
                for (int m = 0; m < 2; ++m) {
                    const uint64_t J = dir ? far[m] - x : x - far[m];
                    CHECK(J <= s, "reach in front of the warm-up start");
                    lb[m] = s - (uint32_t)J;
                }
                const uint32_t lbmin = std::min(lb[0], lb[1]);
                for (int g = 0; g < 2; ++g) {
                    const uint32_t lo = g ? split : 0, hi = g ? n : split, ng = hi - lo;
                    // the model: pair by pair from the rows
                    std::vector<uint32_t> mem(CO.begin() + lo, CO.begin() + hi);
                    const uint64_t C = (uint64_t)ng * (ng ? ng - 1 : 0) / 2;
                    const uint64_t J_range = dir ? S - 1 - x : x;
                    std::vector<uint64_t> surv(J_range + 1, 0);
                    for (uint32_t a = 0; a < ng; ++a)
                        for (uint32_t b = a + 1; b < ng; ++b)
                            for (uint64_t j = 0; j <= J_range; ++j) {
                                const uint64_t xx = dir ? x + j : x - j;
                                if (bit(mem[a], xx) != bit(mem[b], xx)) break;
                                ++surv[j];
                            }
                    Result want{{0, 0}, 0};
                    for (int m = 0; m < 2 && ng >= 2; ++m) {
                        auto dist = [&](uint64_t j) {
                            const uint64_t xx = dir ? x + j : x - j;
                            return m ? j : (posv[xx] > posv[x] ? posv[xx] - posv[x] : posv[x] - posv[xx]);
                        };
                        const uint64_t lim = m ? max_sites : max_bp;
                        uint64_t J_u = 0;
                        for (uint64_t j = 0; j <= J_range; ++j)
                            if (!lim || dist(j) <= lim) J_u = j;
                        if (1000 * surv[0] < (uint64_t)cutoff * C) continue;
                        uint64_t jstar = 0;
                        for (uint64_t j = 0; j <= J_u; ++j)
                            if (1000 * surv[j] >= (uint64_t)cutoff * C) jstar = j;
                        for (uint64_t j = 0; j < jstar; ++j) want.I2[m] += (surv[j] + surv[j + 1]) * (dist(j + 1) - dist(j));
                        if (jstar == J_u) want.flags |= 1u << ((J_u == J_range ? 0 : 8) + 4 * m + 2 * g + dir);
                    }
                    // the code under test
                    Result got{{0, 0}, 0};
                    if (ng >= 2) {
                        std::vector<uint64_t> w(n, 0);
                        uint64_t all = 0;
                        for (uint32_t t = lo + 1; t < hi; ++t) {
                            const uint32_t l = ihs_span_left(t, lo + 1, hi, dval, gm), r = ihs_span_right(t, lo + 1, hi, dval, gm);
                            // plain spans, one break at a time
                            uint32_t pl = 1, pr = 1;
                            for (uint32_t i = t; i > lo + 1 && CD[i - 1] < CD[t]; --i) ++pl;
                            for (uint32_t i = t; i + 1 < hi && CD[i + 1] <= CD[t]; ++i) ++pr;
                            CHECK(l == pl && r == pr, "spans at %u: %u %u want %u %u", t, l, r, pl, pr);
                            w[t] = (uint64_t)l * r;
                            all += w[t];
                        }
                        CHECK(all == C, "weights %llu of %llu pairs", (unsigned long long)all, (unsigned long long)C);
                        auto broken_after = [&](uint32_t xx) {
                            uint64_t a = 0;
                            for (uint32_t t = lo + 1; t < hi; ++t)
                                if (CD[t] > xx) a += w[t];
                            return a;
                        };
                        for (uint32_t xx = 0; xx <= s; ++xx)  // the survivors at every step the walk can see
                            if (s - xx <= J_range) CHECK(C - broken_after(xx) == surv[s - xx], "survivors at step %u", xx);
                        if (ihs_cut_ok(C - broken_after(s), C, cutoff)) {
                            uint32_t xl = lbmin, xh = s;  // the farthest reach first, then bisection
                            if (xl < xh && !ihs_cut_ok(C - broken_after(xl), C, cutoff)) {
                                ++xl;
                                while (xl < xh) {
                                    const uint32_t mid = xl + (xh - xl) / 2;
                                    if (ihs_cut_ok(C - broken_after(mid), C, cutoff)) xh = mid;
                                    else xl = mid + 1;
                                }
                            }
                            for (int m = 0; m < 2; ++m) {
                                const uint32_t e = std::max(xl, lb[m]);
                                auto U = [&](uint32_t step) -> uint64_t {
                                    if (m) return s - step;
                                    const uint64_t q = posv[ordinal(step)];
                                    return q > posv[x] ? q - posv[x] : posv[x] - q;
                                };
                                uint64_t a = 0, b = 0;
                                for (uint32_t t = lo + 1; t < hi; ++t)
                                    if (CD[t] > e) {
                                        a += w[t];
                                        if (CD[t] <= s) b += ihs_break_term(w[t], CD[t], s, U(CD[t]), U(CD[t] - 1));
                                    }
                                got.I2[m] = ihs_alive_term(C - a, U(e)) + b;
                                got.flags |= ihs_flag(m, g, dir, e == lb[m], ihs_far_is_edge(dir, far[m], S));
                            }
                        }
                    }
                    CHECK(got.I2[0] == want.I2[0] && got.I2[1] == want.I2[1] && got.flags == want.flags,
                          "iter %d K %d class %d step %u: got %llu %llu 0x%x want %llu %llu 0x%x", it, K, g, s, (unsigned long long)got.I2[0],
                          (unsigned long long)got.I2[1], got.flags, (unsigned long long)want.I2[0], (unsigned long long)want.I2[1], want.flags);
                }
            }
        }
    }
    printf("ok %d\n", iters);
    return 0;
}
