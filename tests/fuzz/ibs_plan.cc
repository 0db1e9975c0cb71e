// ibs_plan.cc — stand-alone driver for csrc/ibs_plan.h (+ dip_runs.h): the host logic of impop_ibs_scan, run the way ibs.hip runs
// it and compared with a direct scan of the definition.
//   ibs_plan <seed> <rounds>
// Per round: a few pairs with random difference sets over random (optionally compacted) coordinates and a random range; the
// range's 64-site blocks are cut by ibs_cut with random chunk / sub-segment lengths; per sub-segment a DipSummary, combined in
// order with the carried one (the exclusive prefix kept, as the fill sweep does); the fill emulation gives every reported tract a
// slot from ibs_closed_before + a running count.  Checked: pair totals, every tract and its slot, ibs_offsets / ibs_pair_ranges,
// the window tables (ibs_add_tract + IbsWindowPlan::finish) against a per-tract intersection, and the pair tiles.
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <set>
#include <vector>

#include "ibs_plan.h"

using namespace impop;

struct Tract {
    uint64_t s, t;
};

#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            printf("FAIL round %d: ", round);     \
            printf(__VA_ARGS__);                  \
            printf(" (%s:%d)\n", __FILE__, __LINE__); \
            return 1;                             \
        }                                         \
    } while (0)

int main(int argc, char **argv) {
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int rounds = argc > 2 ? atoi(argv[2]) : 200;
    std::mt19937_64 rng(seed);
    auto uni = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };  // inclusive
    const uint32_t mins[5] = {1, 2, 7, 64, 65};
    for (int round = 0; round < rounds; ++round) {
        const uint32_t min_sites = mins[round % 5];
        // columns and their coordinates: dense (coordinate = column) or compacted (strictly increasing, gaps of dropped sites)
        const uint64_t n_col = uni(1, 700);
        const bool compact = uni(0, 2) == 0;
        std::vector<uint64_t> pos(n_col);
        uint64_t x = compact ? uni(0, 50) : 0;
        for (uint64_t c = 0; c < n_col; ++c) {
            pos[c] = x;
            x += compact ? uni(1, uni(0, 3) ? 3 : 200) : 1;
        }
        const uint64_t span = compact ? x + uni(0, 40) : n_col;
        uint64_t b = uni(0, span - 1), e = uni(b + 1, span);
        if (uni(0, 3) == 0) { b = 0; e = span; }
        const uint64_t cb = (uint64_t)(std::lower_bound(pos.begin(), pos.end(), b) - pos.begin());
        const uint64_t ce = (uint64_t)(std::lower_bound(pos.begin(), pos.end(), e) - pos.begin());
        const uint64_t blk0 = cb >> 6, n_blk = ce > cb ? ((ce + 63) >> 6) - blk0 : 0;
        const uint32_t n_pairs = (uint32_t)uni(1, 6);
        const IbsCut cut = ibs_cut(n_blk, 7, n_pairs, 1, (uint32_t)uni(0, 4), uni(0, 1) ? 56 * uni(1, 6) : (1u << 20), (uint32_t)uni(0, 5),
                                   (uint32_t)uni(0, 4));
        CHECK(cut.chunk_blocks >= 1 && cut.seg_blocks >= 1 && cut.n_chunks * cut.chunk_blocks >= n_blk, "cut does not cover");
        CHECK(n_blk == 0 || (cut.n_chunks - 1) * cut.chunk_blocks < n_blk, "an empty chunk");
        CHECK((uint64_t)cut.n_sub * cut.seg_blocks >= cut.chunk_blocks && cut.n_sub <= IBS_MAX_SUB, "sub-segments do not cover a chunk");

        // windows inside the range, some empty, some repeated
        const uint64_t n_win = uni(0, 6);
        std::vector<uint64_t> wb(n_win), we(n_win);
        for (uint64_t i = 0; i < n_win; ++i) {
            wb[i] = uni(b, e);
            we[i] = uni(wb[i], e);
            if (i && uni(0, 4) == 0) { wb[i] = wb[i - 1]; we[i] = we[i - 1]; }
            if (uni(0, 5) == 0) { wb[i] = b; we[i] = e; }
        }
        IbsWindowPlan wp;
        wp.build(wb.data(), we.data(), n_win);
        std::vector<unsigned long long> acc(wp.acc_words() + 1, 0ull);
        IbsWindowsDev wd;
        wd.edge = wp.edge.data();
        wd.sbeg = wp.sbeg.data();
        wd.send = wp.send.data();
        wd.acc = acc.data();
        wd.n_edge = (uint32_t)wp.edge.size();
        wd.n_span = (uint32_t)wp.sbeg.size();
        auto add = [](unsigned long long *p, unsigned long long v) { *p += v; };

        std::vector<uint32_t> n_tracts(n_pairs);
        std::vector<std::vector<Tract>> want_all(n_pairs), got_all(n_pairs);
        for (uint32_t p = 0; p < n_pairs; ++p) {
            // the pair's differing columns inside [cb, ce): none, all, or a random density
            std::vector<uint8_t> diff(n_col, 0);
            const uint64_t mode = uni(0, 5);
            const uint64_t den = mode == 0 ? 0 : mode == 1 ? 1 : uni(2, 120);
            for (uint64_t c = cb; c < ce; ++c) diff[c] = den == 0 ? 0 : den == 1 ? 1 : (rng() % den == 0);
            if (ce > cb && uni(0, 2) == 0) diff[cb] = 1;
            if (ce > cb && uni(0, 2) == 0) diff[ce - 1] = 1;

            // the definition, directly
            uint32_t w_diff = 0, w_longest = 0, w_tracts = 0;
            uint64_t w_sites = 0, prev = b;  // prev: where the tract in progress begins
            std::vector<Tract> &want = want_all[p];
            auto close_at = [&](uint64_t end) {
                const uint64_t len = end - prev;
                if (len > w_longest) w_longest = (uint32_t)len;
                if (len > 0 && len >= min_sites) {
                    ++w_tracts;
                    w_sites += len;
                    want.push_back(Tract{prev, end});
                }
            };
            for (uint64_t c = cb; c < ce; ++c)
                if (diff[c]) {
                    ++w_diff;
                    close_at(pos[c]);
                    prev = pos[c] + 1;
                }
            close_at(e);

            // sweep 1 and 2 as the device runs them
            DipSummary carry = dip_empty();
            std::vector<Tract> &got = got_all[p];
            std::vector<uint32_t> slot_of;
            for (uint64_t c = 0; c < cut.n_chunks; ++c) {
                const uint64_t len = cut.chunk_len(c, n_blk), first = blk0 + cut.chunk_begin(c);
                const uint32_t subs = cut.subs_of(len);
                CHECK(len >= 1 && subs >= 1 && subs <= cut.n_sub, "chunk %llu: %llu blocks in %u sub-segments", (unsigned long long)c,
                      (unsigned long long)len, subs);
                std::vector<DipSummary> sum(subs);
                auto cols_of = [&](uint32_t k, uint64_t &c0, uint64_t &c1) {
                    const uint64_t lb0 = (uint64_t)k * cut.seg_blocks, lb1 = std::min(lb0 + cut.seg_blocks, len);
                    c0 = std::max((first + lb0) * 64, cb);
                    c1 = std::min((first + lb1) * 64, ce);
                };
                for (uint32_t k = 0; k < subs; ++k) {
                    uint64_t c0, c1;
                    cols_of(k, c0, c1);
                    DipSummary s = dip_empty();
                    for (uint64_t col = c0; col < c1; ++col)
                        if (diff[col]) dip_append_site(s, pos[col], min_sites);
                    sum[k] = s;
                }
                DipSummary E = carry;
                for (uint32_t k = 0; k < subs; ++k) {
                    const DipSummary t = sum[k];
                    sum[k] = E;
                    E = dip_combine(E, t, min_sites);
                }
                carry = E;
                for (uint32_t k = 0; k < subs; ++k) {  // the fill walk of sub-segment k
                    uint64_t c0, c1;
                    cols_of(k, c0, c1);
                    DipSummary s = sum[k];
                    uint32_t slot = ibs_closed_before(s, b, min_sites);
                    for (uint64_t col = c0; col < c1; ++col)
                        if (diff[col]) {
                            const uint64_t beg = s.het ? s.last + 1 : b;
                            if (pos[col] - beg >= min_sites) {
                                got.push_back(Tract{beg, pos[col]});
                                slot_of.push_back(slot++);
                            }
                            dip_append_site(s, pos[col], min_sites);
                        }
                }
            }
            const DipSummary closed = dip_close(carry, b, e, min_sites);
            CHECK((uint64_t)closed.run_sum + closed.het == e - b, "pair %u: runs + differences != the range", p);
            CHECK(closed.het == w_diff && closed.longest == w_longest && closed.roh_runs == w_tracts && closed.roh_sites == w_sites,
                  "pair %u: totals %u %u %u %u, want %u %u %u %llu", p, closed.het, closed.longest, closed.roh_runs, closed.roh_sites, w_diff,
                  w_longest, w_tracts, (unsigned long long)w_sites);
            {
                uint32_t slot = ibs_closed_before(carry, b, min_sites);
                const uint64_t beg = carry.het ? carry.last + 1 : b;
                if (e - beg >= min_sites) {
                    got.push_back(Tract{beg, e});
                    slot_of.push_back(slot++);
                }
                CHECK(slot == w_tracts, "pair %u: %u slots for %u tracts", p, slot, w_tracts);
            }
            CHECK(got.size() == want.size(), "pair %u: %zu tracts, want %zu", p, got.size(), want.size());
            for (size_t i = 0; i < got.size(); ++i)
                CHECK(slot_of[i] == i && got[i].s == want[i].s && got[i].t == want[i].t, "pair %u tract %zu: [%llu,%llu) slot %u, want [%llu,%llu)",
                      p, i, (unsigned long long)got[i].s, (unsigned long long)got[i].t, slot_of[i], (unsigned long long)want[i].s,
                      (unsigned long long)want[i].t);
            n_tracts[p] = w_tracts;
            for (const Tract &t : got) ibs_add_tract(wd, t.s, t.t, add);
        }

        // offsets and the pair ranges of a staging
        const std::vector<uint64_t> off = ibs_offsets(n_pairs, [&](uint64_t p) { return n_tracts[p]; });
        uint64_t total = 0;
        for (uint32_t p = 0; p < n_pairs; ++p) {
            CHECK(off[p] == total, "offset of pair %u", p);
            total += n_tracts[p];
        }
        CHECK(off[n_pairs] == total, "total");
        const uint64_t cap = uni(1, 12);
        const std::vector<uint64_t> ranges = ibs_pair_ranges(off, cap);
        CHECK(ranges.front() == 0 && ranges.back() == n_pairs, "ranges do not cover the pairs");
        for (size_t k = 0; k + 1 < ranges.size(); ++k) {
            CHECK(ranges[k] < ranges[k + 1], "an empty pair range");
            CHECK(off[ranges[k + 1]] - off[ranges[k]] <= cap || ranges[k + 1] == ranges[k] + 1, "a range of several pairs exceeds the staging");
        }

        // window records against a per-tract intersection
        CHECK(acc[wp.acc_words()] == 0, "the tables were written past their end");
        const std::vector<IbsWindowSums> sums = wp.finish(acc.data());
        for (uint64_t i = 0; i < n_win; ++i) {
            uint64_t sites = 0, meets = 0, spans = 0;
            if (we[i] > wb[i])
                for (uint32_t p = 0; p < n_pairs; ++p)
                    for (const Tract &t : want_all[p]) {
                        const uint64_t lo = std::max(t.s, wb[i]), hi = std::min(t.t, we[i]);
                        if (hi > lo) sites += hi - lo;
                        meets += t.s < we[i] && t.t > wb[i];
                        spans += t.s <= wb[i] && t.t >= we[i];
                    }
            CHECK(sums[i].pair_sites == sites && sums[i].tracts == meets && sums[i].spanning == spans,
                  "window %llu [%llu,%llu): %llu %llu %llu, want %llu %llu %llu", (unsigned long long)i, (unsigned long long)wb[i],
                  (unsigned long long)we[i], (unsigned long long)sums[i].pair_sites, (unsigned long long)sums[i].tracts,
                  (unsigned long long)sums[i].spanning, (unsigned long long)sites, (unsigned long long)meets, (unsigned long long)spans);
        }

        // pair tiles: every pair of [p0, p1) lies in exactly one listed tile; pair indices are i-major
        {
            const uint32_t n = (uint32_t)uni(2, 70);
            const uint64_t np = (uint64_t)n * (n - 1) / 2;
            uint64_t idx = 0;
            for (uint32_t i = 0; i < n; ++i)
                for (uint32_t j = i + 1; j < n; ++j) CHECK(ibs_pair_index(n, i, j) == idx++, "pair index (%u,%u) of %u", i, j, n);
            const uint64_t p0 = uni(0, np - 1), p1 = uni(0, 3) ? uni(p0 + 1, np) : np;
            const std::vector<IbsTile> tiles = ibs_tiles_all(n, p0, p1);
            std::vector<uint32_t> seen(np, 0);
            for (const IbsTile &t : tiles) {
                CHECK(t.a0 <= t.b0, "tile order");
                uint64_t lo = np, hi = 0;
                for (uint32_t a = t.a0 * IBS_TILE; a < (t.a0 + 1) * IBS_TILE; ++a)
                    for (uint32_t c = t.b0 * IBS_TILE; c < (t.b0 + 1) * IBS_TILE; ++c)
                        if (a < c && c < n) {
                            const uint64_t q = ibs_pair_index(n, a, c);
                            seen[q] += 1;
                            lo = std::min(lo, q);
                            hi = std::max(hi, q);
                        }
                CHECK(lo <= hi && hi >= p0 && lo < p1, "tile (%u,%u) lies outside the range", t.a0, t.b0);
            }
            for (uint64_t q = 0; q < np; ++q) CHECK(seen[q] <= 1 && (q < p0 || q >= p1 || seen[q] == 1), "pair %llu in %u tiles", (unsigned long long)q, seen[q]);
            const std::vector<IbsTile> lt = ibs_tiles_list(p0, p1);
            CHECK(!lt.empty() && (uint64_t)lt.front().a0 * IBS_PAIRS <= p0 && ((uint64_t)lt.back().a0 + 1) * IBS_PAIRS >= p1 &&
                      lt.size() == lt.back().a0 - lt.front().a0 + 1u,
                  "list tiles");
        }
    }
    printf("ok %d\n", rounds);
    return 0;
}
