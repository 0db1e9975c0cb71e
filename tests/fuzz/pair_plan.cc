// Host check of csrc/pair_plan.h (plain C++, built with the host sanitizers by tests/test_host_logic.py).
//     pair_plan CAP WIN_CAP  b0 e0  b1 e1 ...
// plans the windows [b, e), walks the chunks and checks both against a brute-force model computed here, site by site.
// Exit 0 and one line — "plan segmented=S cells=C chunks=K", or "too_wide window=I cells=N" when the walk reports a window
// that spans more cells than fit — else exit 1 with the breached property on stderr.
//
// What "empty" means for the plan: a window without sites needs no Gram matrix.  In a segmented plan it has count == 0 and
// comes last in `ord`.  In an unsegmented plan cell i IS window i for every i, so an empty window owns one cell of zero sites
// (count == 1) and stays where it was: that keeps a tiling with an empty window a one-matrix-per-problem batch.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "pair_plan.h"

struct Win {
    uint64_t site_begin, site_end;
};

#define CHECK(cond, ...)              \
    do {                              \
        if (!(cond)) {                \
            fprintf(stderr, "BREACH %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__); \
            fprintf(stderr, "\n");    \
            return 1;                 \
        }                             \
    } while (0)

int main(int argc, char **argv) {
    if (argc < 3 || (argc - 3) % 2) return 2;
    const uint64_t cap = strtoull(argv[1], nullptr, 10), win_cap = strtoull(argv[2], nullptr, 10);
    if (!cap || !win_cap) return 2;
    std::vector<Win> w;
    uint64_t span = 0;
    for (int i = 3; i + 1 < argc; i += 2) {
        w.push_back({strtoull(argv[i], nullptr, 10), strtoull(argv[i + 1], nullptr, 10)});
        if (w.back().site_end < w.back().site_begin) return 2;
        span = std::max(span, w.back().site_end);
    }
    const uint64_t n = w.size();
    impop::PairPlan p;
    CHECK(impop::plan_cells(w.data(), n, p), "a short list was refused");
    CHECK(p.first.size() == n && p.count.size() == n && p.ord.size() == n, "table sizes");

    // ---- the model: how many windows cover each site
    std::vector<uint32_t> cover(span + 1, 0);
    uint64_t win_sites = 0, covered = 0;
    for (const Win &x : w)
        for (uint64_t s = x.site_begin; s < x.site_end; ++s) { ++cover[s]; ++win_sites; }
    for (uint64_t s = 0; s < span; ++s) covered += cover[s] > 0;
    CHECK(p.segmented == (covered * 20 < win_sites * 19), "segmented=%d with %llu of %llu sites", (int)p.segmented,
          (unsigned long long)covered, (unsigned long long)win_sites);

    // ---- cells
    uint64_t cell_sites = 0;
    if (!p.segmented) {
        CHECK(p.cells.size() == n, "unsegmented: %zu cells for %llu windows", p.cells.size(), (unsigned long long)n);
        for (uint64_t i = 0; i < n; ++i) {
            CHECK(p.cells[i].b == w[i].site_begin && p.cells[i].e == w[i].site_end, "unsegmented: cell %llu is not window %llu", (unsigned long long)i, (unsigned long long)i);
            CHECK(p.first[i] == i && p.count[i] == 1, "unsegmented: window %llu -> cells [%u, +%u)", (unsigned long long)i, p.first[i], p.count[i]);
            CHECK(p.ord[i] == i, "unsegmented: ord is not the caller's order");
        }
    } else {
        for (size_t c = 0; c < p.cells.size(); ++c) {
            CHECK(p.cells[c].b < p.cells[c].e, "cell %zu is empty", c);
            CHECK(c == 0 || p.cells[c - 1].e <= p.cells[c].b, "cells %zu, %zu overlap or are unsorted", c - 1, c);
            for (uint64_t s = p.cells[c].b; s < p.cells[c].e; ++s) CHECK(s < span && cover[s] > 0, "site %llu of cell %zu is in no window", (unsigned long long)s, c);
            cell_sites += p.cells[c].e - p.cells[c].b;
        }
        CHECK(cell_sites == covered, "cells hold %llu sites, windows cover %llu", (unsigned long long)cell_sites, (unsigned long long)covered);
        CHECK(cell_sites * 20 < win_sites * 19, "segmented without 5 %% shared");
    }
    for (uint64_t i = 0; i < n; ++i) {
        if (w[i].site_end == w[i].site_begin) {
            if (p.segmented) CHECK(p.count[i] == 0, "empty window %llu has %u cells", (unsigned long long)i, p.count[i]);
            continue;
        }
        CHECK(p.count[i] >= 1 && (uint64_t)p.first[i] + p.count[i] <= p.cells.size(), "window %llu -> cells [%u, +%u) of %zu",
              (unsigned long long)i, p.first[i], p.count[i], p.cells.size());
        uint64_t at = w[i].site_begin;  // contiguous cells whose union is exactly the window
        for (uint32_t c = p.first[i]; c < p.first[i] + p.count[i]; ++c) {
            CHECK(p.cells[c].b == at, "window %llu: cell %u starts at %llu, expected %llu", (unsigned long long)i, c, (unsigned long long)p.cells[c].b, (unsigned long long)at);
            at = p.cells[c].e;
        }
        CHECK(at == w[i].site_end, "window %llu: its cells end at %llu", (unsigned long long)i, (unsigned long long)at);
    }

    // ---- order: a permutation, windows without cells last, segmented: the others by first cell, ties in the caller's order
    std::vector<int> seen(n, 0);
    for (uint64_t k = 0; k < n; ++k) {
        CHECK(p.ord[k] < n && !seen[p.ord[k]]++, "ord is no permutation at %llu", (unsigned long long)k);
        if (!k) continue;
        const uint64_t a = p.ord[k - 1], b = p.ord[k];
        CHECK(p.count[a] != 0 || p.count[b] == 0, "a window with cells follows one without at %llu", (unsigned long long)k);
        if (p.segmented && p.count[b]) CHECK(p.first[a] < p.first[b] || (p.first[a] == p.first[b] && a < b), "ord is not sorted at %llu", (unsigned long long)k);
    }

    // ---- chunks
    impop::PairChunkWalk walk(p, cap, win_cap);
    impop::PairChunkSpan c;
    uint64_t next = 0, chunks = 0;
    for (;;) {
        const impop::PairChunkWalk::Step step = walk.next(c);
        if (step == impop::PairChunkWalk::DONE) break;
        if (step == impop::PairChunkWalk::TOO_WIDE) {
            CHECK(next < n && walk.bad_window == p.ord[next], "too wide: window %llu is not the next one", (unsigned long long)walk.bad_window);
            CHECK(walk.bad_cells == p.count[walk.bad_window] && walk.bad_cells > cap, "too wide: %u cells against a capacity of %llu", walk.bad_cells, (unsigned long long)cap);
            printf("too_wide window=%llu cells=%u\n", (unsigned long long)walk.bad_window, walk.bad_cells);
            return 0;
        }
        ++chunks;
        CHECK(c.base == next && c.cnt >= 1 && c.cnt <= win_cap && c.base + c.cnt <= n, "chunk [%llu, +%llu) after %llu windows",
              (unsigned long long)c.base, (unsigned long long)c.cnt, (unsigned long long)next);
        uint64_t lo = ~0ull, hi = 0;  // the cells the chunk's windows touch
        bool one = true;
        for (uint64_t k = 0; k < c.cnt; ++k) {
            const uint64_t i = p.ord[c.base + k];
            if (p.count[i]) { lo = std::min<uint64_t>(lo, p.first[i]); hi = std::max<uint64_t>(hi, (uint64_t)p.first[i] + p.count[i]); }
        }
        if (hi == 0) CHECK(c.n_cells == 0, "a chunk of windows without cells has %u", c.n_cells);
        else CHECK(c.c_lo == lo && c.n_cells == hi - lo, "chunk cells [%u, +%u), its windows touch [%llu, %llu)", c.c_lo, c.n_cells, (unsigned long long)lo, (unsigned long long)hi);
        CHECK(c.n_cells <= cap && (uint64_t)c.c_lo + c.n_cells <= p.cells.size(), "chunk of %u cells, capacity %llu", c.n_cells, (unsigned long long)cap);
        for (uint64_t k = 0; k < c.cnt; ++k) {
            const uint64_t i = p.ord[c.base + k];
            const uint32_t fv = c.first_of(p, i), cv = p.count[i];  // what goes to the device as seg_first / seg_count
            CHECK((uint64_t)fv + cv <= c.n_cells, "window %llu reads Gram matrices [%u, +%u) of the chunk's %u", (unsigned long long)i, fv, cv, c.n_cells);
            if (cv) CHECK(c.c_lo + fv == p.first[i], "window %llu starts at the wrong matrix", (unsigned long long)i);
            one = one && cv == 1 && fv == k;
        }
        CHECK(c.one_to_one(p) == one, "one_to_one=%d, model %d", (int)c.one_to_one(p), (int)one);
        next += c.cnt;
    }
    CHECK(next == n, "the chunks hold %llu of %llu windows", (unsigned long long)next, (unsigned long long)n);
    for (uint64_t i = 0; i < n; ++i) CHECK(p.count[i] <= cap, "window %llu spans %u cells, capacity %llu, and the walk went through", (unsigned long long)i, p.count[i], (unsigned long long)cap);
    printf("plan segmented=%d cells=%zu chunks=%llu\n", (int)p.segmented, p.cells.size(), (unsigned long long)chunks);
    return 0;
}
