// paint_math.cc — stand-alone driver for csrc/paint_math.h (no HIP): builds with a host compiler under ASan + UBSan.
//   paint_math <seed> <rounds>
// Every round draws K donors, L sites, a mismatch cost mu and switch costs c_s and runs two things side by side:
//   the device's form   K states (R, T) driven by paint_site_update, the site minimum taken as the minimum of paint_pack words,
//                       paint_renorm, the 64-bit cost as the sum of the minima, one PaintRec per site, paint_backtrack;
//   the definition      the literal recursion of include/impop_hip.h in 64-bit integers with the full table of stay bits,
//                       d(L-1) = A(L-1), d(s-1) = d(s) if stay_{d(s)}(s) else A(s-1).
// and compares the cost, A(s) at every site, the path at every site and the segment count; R is checked to stay within
// c_s + mu at every step.  The draws include c_s = 0, mu = c, all-equal rows, duplicated donors, K = 1 and K = 1024, per-site costs
// with zeros, and one long round at the limits (mu = 65535, c = 2^20) over more than 2^16 sites, where the cost passes 2^32.
// paint_overlap is compared with a count of the sites.  Prints "ok <rounds>" or the first difference.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "paint_math.h"

using namespace impop;

struct Draw {
    uint32_t K, L, mu;
    std::vector<uint32_t> cs;          // c_s, cs[0] unused
    std::vector<uint8_t> x;            // [L]
    std::vector<uint8_t> d;            // [K][L]
};

static int run(const Draw &w, const char *tag) {
    const uint32_t K = w.K, L = w.L;
    // the definition
    std::vector<uint64_t> V(K), Vn(K);
    std::vector<uint8_t> stay((size_t)K * L, 0);
    std::vector<uint32_t> A(L);
    std::vector<uint64_t> M(L);
    for (uint32_t j = 0; j < K; ++j) V[j] = w.d[(size_t)j * L] != w.x[0] ? w.mu : 0;
    auto argmin = [&](const std::vector<uint64_t> &v, uint64_t &mn) {
        uint32_t a = 0;
        for (uint32_t j = 1; j < K; ++j)
            if (v[j] < v[a]) a = j;
        mn = v[a];
        return a;
    };
    A[0] = argmin(V, M[0]);
    // the device's form
    std::vector<uint32_t> R(K, 0u), T(K, 0u);
    std::vector<PaintRec> rec(L);
    uint64_t cost = 0;
    for (uint32_t s = 0; s < L; ++s) {
        const uint32_t c = s == 0 ? 0u : w.cs[s];
        if (s > 0) {
            const uint64_t sw = M[s - 1] + c;
            for (uint32_t j = 0; j < K; ++j) {
                stay[(size_t)j * L + s] = V[j] <= sw;
                Vn[j] = (w.d[(size_t)j * L + s] != w.x[s] ? w.mu : 0) + (V[j] <= sw ? V[j] : sw);
            }
            V.swap(Vn);
            A[s] = argmin(V, M[s]);
        }
        uint32_t best = 0xFFFFFFFFu, best_org = 0;
        for (uint32_t j = 0; j < K; ++j) {
            paint_site_update(R[j], T[j], c, w.d[(size_t)j * L + s] != w.x[s], w.mu, s);
            if (R[j] > c + w.mu || R[j] >= PAINT_IDLE) {
                printf("%s: R out of range at site %u state %u: %u\n", tag, s, j, R[j]);
                return 1;
            }
            const uint32_t p = paint_pack(R[j], j);
            if (p < best) {
                best = p;
                best_org = T[j];
            }
        }
        if (paint_pack(PAINT_IDLE, PAINT_MAX_DONORS - 1) <= best) {
            printf("%s: an idle slot would win at site %u\n", tag, s);
            return 1;
        }
        const uint32_t mn = paint_pack_value(best);
        cost += mn;
        rec[s] = PaintRec{paint_pack_slot(best), best_org};
        for (uint32_t j = 0; j < K; ++j) paint_renorm(R[j], mn);
        if (rec[s].slot != A[s] || cost != M[s]) {
            printf("%s: site %u: A %u / %u, cost %llu / %llu\n", tag, s, rec[s].slot, A[s], (unsigned long long)cost, (unsigned long long)M[s]);
            return 1;
        }
    }
    // the paths
    std::vector<uint32_t> want(L), got(L, 0xFFFFFFFFu);
    want[L - 1] = A[L - 1];
    for (uint32_t s = L - 1; s > 0; --s) want[s - 1] = stay[(size_t)want[s] * L + s] ? want[s] : A[s - 1];
    uint32_t want_segs = 1;
    for (uint32_t s = 1; s < L; ++s) want_segs += want[s] != want[s - 1];
    uint32_t last_begin = L;
    bool order = true;
    const uint32_t n = paint_backtrack(rec.data(), L, L, [&](uint32_t, uint32_t slot, uint32_t s0, uint32_t s1) {
        order = order && s1 == last_begin && s0 < s1;
        last_begin = s0;
        for (uint32_t s = s0; s < s1; ++s) got[s] = slot;
    });
    if (n != want_segs || !order || last_begin != 0) {
        printf("%s: %u segments, the definition has %u (order %d, first begin %u)\n", tag, n, want_segs, (int)order, last_begin);
        return 1;
    }
    for (uint32_t s = 0; s < L; ++s)
        if (got[s] != want[s]) {
            printf("%s: path differs at site %u: %u / %u\n", tag, s, got[s], want[s]);
            return 1;
        }
    // a bound below the count stops the walk and says so; nothing is emitted past it
    if (want_segs > 1) {
        uint32_t calls = 0;
        const uint32_t m = paint_backtrack(rec.data(), L, want_segs - 1, [&](uint32_t k, uint32_t, uint32_t, uint32_t) { calls += k < want_segs - 1; });
        if (m != want_segs || calls != want_segs - 1) {
            printf("%s: bounded walk returned %u after %u calls\n", tag, m, calls);
            return 1;
        }
    }
    return 0;
}

static Draw draw(std::mt19937_64 &rng, uint32_t K, uint32_t L, uint32_t mu, int cost_kind, uint32_t c, int rows_kind) {
    Draw w;
    w.K = K;
    w.L = L;
    w.mu = mu;
    w.cs.assign(L, c);
    if (cost_kind == 1)
        for (auto &v : w.cs) v = (uint32_t)(rng() % 4) == 0 ? 0u : (uint32_t)(rng() % (2 * (uint64_t)mu + 2));
    if (cost_kind == 2)
        for (auto &v : w.cs) v = (uint32_t)(rng() % 3) == 0 ? PAINT_MAX_COST : (uint32_t)(rng() % 3);
    w.x.resize(L);
    w.d.resize((size_t)K * L);
    // founders with switches: ties and real mosaics
    const uint32_t nf = 1 + (uint32_t)(rng() % 4);
    std::vector<uint8_t> f((size_t)nf * L);
    for (auto &v : f) v = (uint8_t)(rng() & 1);
    auto fill = [&](uint8_t *row) {
        uint32_t cur = (uint32_t)(rng() % nf);
        for (uint32_t s = 0; s < L; ++s) {
            if (rng() % 16 == 0) cur = (uint32_t)(rng() % nf);
            row[s] = f[(size_t)cur * L + s] ^ (uint8_t)(rng() % 32 == 0);
        }
    };
    fill(w.x.data());
    for (uint32_t j = 0; j < K; ++j) {
        if (rows_kind == 1) std::copy(w.x.begin(), w.x.end(), w.d.begin() + (size_t)j * L);          // all equal to the recipient
        else if (rows_kind == 2 && j > 0 && rng() % 2) std::copy(w.d.begin(), w.d.begin() + L, w.d.begin() + (size_t)j * L);  // duplicates
        else fill(w.d.data() + (size_t)j * L);
    }
    return w;
}

int main(int argc, char **argv) {
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int rounds = argc > 2 ? atoi(argv[2]) : 100;
    std::mt19937_64 rng(seed);
    const uint32_t KS[8] = {1, 2, 3, 5, 17, 64, 65, 1024};
    for (int r = 0; r < rounds; ++r) {
        const uint32_t K = KS[r % 8], L = K == 1024 ? 1 + (uint32_t)(rng() % 40) : 1 + (uint32_t)(rng() % 200);
        const uint32_t mu = r % 5 == 0 ? PAINT_MAX_MU : 1 + (uint32_t)(rng() % 4);
        const int cost_kind = r % 3;
        uint32_t c = r % 7 == 0 ? 0u : r % 7 == 1 ? mu : r % 7 == 2 ? PAINT_MAX_COST : (uint32_t)(rng() % 6);
        char tag[96];
        snprintf(tag, sizeof tag, "round %d (K %u L %u mu %u cost_kind %d c %u)", r, K, L, mu, cost_kind, c);
        if (run(draw(rng, K, L, mu, cost_kind, c, (r / 8) % 3), tag)) return 1;
    }
    // the limits over more than 2^16 sites: complementary rows, so every site costs mu or a switch and the cost passes 2^32
    {
        Draw w = draw(rng, 3, 70000, PAINT_MAX_MU, 0, PAINT_MAX_COST, 0);
        for (uint32_t s = 0; s < w.L; ++s) w.d[s] = w.d[(size_t)w.L + s] = w.d[2 * (size_t)w.L + s] = (uint8_t)!w.x[s];
        if (run(w, "limits, all mismatch")) return 1;
        Draw v = draw(rng, 4, 66000, PAINT_MAX_MU, 2, 0, 0);
        if (run(v, "limits, per-site costs")) return 1;
    }
    // paint_overlap against a count
    for (int r = 0; r < 2000; ++r) {
        const uint32_t s0 = (uint32_t)(rng() % 40), s1 = s0 + (uint32_t)(rng() % 40), w0 = (uint32_t)(rng() % 60), w1 = w0 + (uint32_t)(rng() % 40);
        uint32_t n = 0;
        for (uint32_t s = s0; s < s1; ++s) n += s >= w0 && s < w1;
        if (paint_overlap(s0, s1, w0, w1) != n) {
            printf("overlap [%u,%u) x [%u,%u): %u / %u\n", s0, s1, w0, w1, paint_overlap(s0, s1, w0, w1), n);
            return 1;
        }
    }
    printf("ok %d\n", rounds);
    return 0;
}
