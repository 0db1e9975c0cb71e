// Host check of csrc/panel_set.h (plain C++, built with the host sanitizers by tests/test_panel_set_host.py).
//     panel_set SEED ROUNDS
//         n_hap in {1, 2, 63, 64, 65, 130} x K in 1 .. 8 x ROUNDS seeded random sets of disjoint masks (one-member panels and
//         haplotypes in no panel among them, the masks' spare bits above n_hap set), each checked against a brute-force model
//         computed here: the members of a mask by a bit loop, a pair's list as the sorted union, z0 from membership.  Then the
//         refusals: every set once more with one member given to a second mask, and once more with one mask emptied.
//         "panel_set ok sets=N refusals=M"
// Exit 0, else exit 1 with the breached property on stderr.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "panel_set.h"

#define CHECK(cond, ...)                                                      \
    do {                                                                      \
        if (!(cond)) {                                                        \
            fprintf(stderr, "BREACH %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                                     \
            fprintf(stderr, "\n");                                            \
            return 1;                                                         \
        }                                                                     \
    } while (0)

static uint64_t g_rng;
static uint64_t rnd(uint64_t below) {  // splitmix64
    uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (z ^ (z >> 31)) % below;
}

struct Masks {
    uint32_t n_hap, K, mwords;
    std::vector<uint64_t> w;  // K x mwords
    bool has(uint32_t k, uint32_t i) const { return (w[(size_t)k * mwords + (i >> 6)] >> (i & 63)) & 1ull; }
    void set(uint32_t k, uint32_t i, bool on) {
        uint64_t &x = w[(size_t)k * mwords + (i >> 6)];
        x = on ? x | (1ull << (i & 63)) : x & ~(1ull << (i & 63));
    }
};

// the model's members of mask k: a bit loop over the haplotypes, nothing else
static std::vector<uint32_t> model_members(const Masks &m, uint32_t k) {
    std::vector<uint32_t> out;
    for (uint32_t i = 0; i < m.n_hap; ++i)
        if (m.has(k, i)) out.push_back(i);
    return out;
}

// the model's refusal: the populations in turn, each one's members ascending against the owners so far, then its emptiness
static impop::PanelRefusal model_refusal(const Masks &m) {
    std::vector<int> owner(m.n_hap, -1);
    impop::PanelRefusal r;
    for (uint32_t k = 0; k < m.K; ++k) {
        const std::vector<uint32_t> mem = model_members(m, k);
        for (uint32_t i : mem) {
            if (owner[i] >= 0) {
                r.kind = impop::PanelRefusal::OVERLAP; r.k = k; r.other = (uint32_t)owner[i];
                return r;
            }
            owner[i] = (int)k;
        }
        if (mem.empty()) {
            r.kind = impop::PanelRefusal::EMPTY; r.k = k;
            return r;
        }
    }
    return r;
}

static int check_set(const Masks &m) {
    impop::PanelSet P;
    const impop::PanelRefusal r = impop::panel_set(m.w.data(), m.K, m.n_hap, P);
    CHECK(r.kind == impop::PanelRefusal::NONE, "n_hap %u K %u: a disjoint set was refused (kind %d, %u, %u)", m.n_hap, m.K, (int)r.kind, r.k, r.other);
    // classes, positions, offsets and sizes
    std::vector<std::vector<uint32_t>> mem(m.K);
    std::vector<uint8_t> cls(m.n_hap, 0xFF);
    uint32_t M = 0;
    CHECK(P.K == m.K && P.cls.size() == m.n_hap && P.sizes.size() == m.K, "n_hap %u K %u: sizes of the tables", m.n_hap, m.K);
    for (uint32_t k = 0; k < m.K; ++k) {
        mem[k] = model_members(m, k);
        CHECK(P.off[k] == M && P.sizes[k] == mem[k].size() && P.size(k) == mem[k].size(), "n_hap %u K %u: panel %u at %u with %u members, model %u with %zu",
              m.n_hap, m.K, k, P.off[k], P.sizes[k], M, mem[k].size());
        for (uint32_t i : mem[k]) {
            cls[i] = (uint8_t)k;
            CHECK(M < P.hap_of.size() && P.hap_of[M] == i, "n_hap %u K %u: position %u is not haplotype %u", m.n_hap, m.K, M, i);
            ++M;
        }
    }
    CHECK(P.M == M && P.hap_of.size() == M, "n_hap %u K %u: M %u, model %u", m.n_hap, m.K, P.M, M);
    for (uint32_t k = m.K; k <= 8; ++k) CHECK(P.off[k] == M, "n_hap %u K %u: off[%u] = %u, not M = %u", m.n_hap, m.K, k, P.off[k], M);
    CHECK(P.cls == cls, "n_hap %u K %u: classes", m.n_hap, m.K);
    // the merged lists, with and without the observed labelling
    const uint32_t NP = m.K * (m.K - 1) / 2;
    uint32_t m_max = 0;
    for (uint32_t a = 0; a < m.K; ++a)
        for (uint32_t b = a + 1; b < m.K; ++b) m_max = std::max<uint32_t>(m_max, (uint32_t)(mem[a].size() + mem[b].size()));
    for (int with_z0 = 0; with_z0 < 2; ++with_z0) {
        const impop::MergedPairs R = impop::merged_pairs(P, with_z0 != 0);
        CHECK(R.moff.size() == NP + 1 && R.moff[0] == 0, "n_hap %u K %u: moff holds %zu entries", m.n_hap, m.K, R.moff.size());
        CHECK(R.m_max == m_max && R.mw_max == (m_max + 63) / 64, "n_hap %u K %u: m_max %u / mw_max %u, model %u", m.n_hap, m.K, R.m_max, R.mw_max, m_max);
        CHECK(R.z0.size() == (with_z0 ? (size_t)NP * R.mw_max : 0), "n_hap %u K %u: z0 holds %zu words", m.n_hap, m.K, R.z0.size());
        uint64_t total = 0;
        for (uint32_t a = 0, p = 0; a < m.K; ++a)
            for (uint32_t b = a + 1; b < m.K; ++b, ++p) {
                std::vector<uint32_t> both(mem[a]);  // the model: the union, sorted by haplotype index
                both.insert(both.end(), mem[b].begin(), mem[b].end());
                std::sort(both.begin(), both.end());
                CHECK(R.moff[p] == total && R.moff[p + 1] - R.moff[p] == both.size(), "n_hap %u K %u: pair %u at %u .. %u, model %llu + %zu", m.n_hap,
                      m.K, p, R.moff[p], R.moff[p + 1], (unsigned long long)total, both.size());
                for (size_t at = 0; at < both.size(); ++at) {
                    const uint32_t pos = R.merged[R.moff[p] + at];
                    CHECK(pos < M && P.hap_of[pos] == both[at], "n_hap %u K %u: pair %u entry %zu is not haplotype %u", m.n_hap, m.K, p, at, both[at]);
                    const bool in_a = m.has(a, both[at]);
                    CHECK(in_a ? (pos >= P.off[a] && pos < P.off[a + 1]) : (pos >= P.off[b] && pos < P.off[b + 1]),
                          "n_hap %u K %u: pair %u entry %zu: position %u lies in the wrong panel", m.n_hap, m.K, p, at, pos);
                    if (with_z0)
                        CHECK((bool)((R.z0[(size_t)p * R.mw_max + (at >> 6)] >> (at & 63)) & 1ull) == in_a, "n_hap %u K %u: pair %u: z0 bit %zu", m.n_hap,
                              m.K, p, at);
                }
                if (with_z0)
                    for (size_t bit = both.size(); bit < (size_t)R.mw_max * 64; ++bit)  // the rest of the last word, and every word beyond it
                        CHECK(!((R.z0[(size_t)p * R.mw_max + (bit >> 6)] >> (bit & 63)) & 1ull), "n_hap %u K %u: pair %u: z0 bit %zu beyond its %zu members",
                              m.n_hap, m.K, p, bit, both.size());
                total += both.size();
            }
        CHECK(R.moff[NP] == total && R.merged.size() == total, "n_hap %u K %u: moff[NP] %u, the pairs hold %llu", m.n_hap, m.K, R.moff[NP],
              (unsigned long long)total);
    }
    return 0;
}

static int check_refusal(const Masks &m, impop::PanelRefusal::Kind kind, uint32_t k, uint32_t other) {
    impop::PanelSet P;
    const impop::PanelRefusal r = impop::panel_set(m.w.data(), m.K, m.n_hap, P), want = model_refusal(m);
    CHECK(want.kind == kind && want.k == k && (kind != impop::PanelRefusal::OVERLAP || want.other == other),
          "n_hap %u K %u: the model refuses (%d, %u, %u), the case was built for (%d, %u, %u)", m.n_hap, m.K, (int)want.kind, want.k, want.other, (int)kind, k,
          other);
    CHECK(r.kind == kind && r.k == k && (kind != impop::PanelRefusal::OVERLAP || r.other == other), "n_hap %u K %u: refused as (%d, %u, %u), not (%d, %u, %u)",
          m.n_hap, m.K, (int)r.kind, r.k, r.other, (int)kind, k, other);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: panel_set SEED ROUNDS\n");
        return 2;
    }
    g_rng = strtoull(argv[1], nullptr, 10);
    const int rounds = atoi(argv[2]);
    const uint32_t sizes[] = {1, 2, 63, 64, 65, 130};
    int sets = 0, refusals = 0;
    for (uint32_t n_hap : sizes)
        for (uint32_t K = 1; K <= 8; ++K) {
            Masks everyone{n_hap, K, (n_hap + 63) / 64, {}};
            {  // no masks at all: every population is everyone
                impop::PanelSet P;
                const impop::PanelRefusal r = impop::panel_set(nullptr, K, n_hap, P);
                if (K == 1) CHECK(r.kind == impop::PanelRefusal::NONE && P.M == n_hap && P.off[1] == n_hap, "n_hap %u: null masks, K = 1", n_hap);
                else CHECK(r.kind == impop::PanelRefusal::OVERLAP && r.k == 1 && r.other == 0, "n_hap %u K %u: null masks must overlap as (1, 0)", n_hap, K);
                ++refusals;
            }
            if (K > n_hap) {  // no K disjoint panels exist: whatever the masks, some population is refused; here the last is empty
                Masks m = everyone;
                m.w.assign((size_t)K * m.mwords, 0ull);
                for (uint32_t k = 0; k < n_hap; ++k) m.set(k, k, true);
                if (check_refusal(m, impop::PanelRefusal::EMPTY, n_hap, 0)) return 1;
                ++refusals;
                continue;
            }
            for (int round = 0; round < rounds; ++round) {
                Masks m = everyone;
                m.w.assign((size_t)K * m.mwords, 0ull);
                // every panel gets one member first, then the others go to a panel or (one in four) to none; every third round keeps
                // panel `lone` at its one member
                std::vector<uint32_t> order(n_hap);
                for (uint32_t i = 0; i < n_hap; ++i) order[i] = i;
                for (uint32_t i = n_hap; i > 1; --i) std::swap(order[i - 1], order[rnd(i)]);
                const uint32_t lone = round % 3 == 0 ? (uint32_t)rnd(K) : K;
                for (uint32_t k = 0; k < K; ++k) m.set(k, order[k], true);
                for (uint32_t j = K; j < n_hap; ++j) {
                    const uint32_t k = (uint32_t)rnd(K);
                    if (rnd(4) != 0 && k != lone) m.set(k, order[j], true);
                }
                for (uint32_t k = 0; k < K; ++k)  // the spare bits of the last word: they are nobody
                    for (uint32_t bit = n_hap; bit < m.mwords * 64; ++bit) m.set(k, bit, true);
                if (check_set(m)) return 1;
                ++sets;
                if (K >= 2) {  // a member of population `from` also given to population `to`: refused at the later of the two
                    const uint32_t from = (uint32_t)rnd(K), to = (from + 1 + (uint32_t)rnd(K - 1)) % K;
                    Masks o = m;
                    o.set(to, model_members(m, from)[rnd(model_members(m, from).size())], true);
                    if (check_refusal(o, impop::PanelRefusal::OVERLAP, std::max(from, to), std::min(from, to))) return 1;
                    ++refusals;
                }
                Masks e = m;  // one population emptied (its spare bits stay set)
                const uint32_t k = (uint32_t)rnd(K);
                for (uint32_t i = 0; i < n_hap; ++i) e.set(k, i, false);
                if (check_refusal(e, impop::PanelRefusal::EMPTY, k, 0)) return 1;
                ++refusals;
            }
        }
    printf("panel_set ok sets=%d refusals=%d\n", sets, refusals);
    return 0;
}
