// pair_plan.h — the index arithmetic of the windowed all-pairs calls (pairwise_scan.hip pairwise_front): which Gram cells a window
// list needs, and which windows go into which chunk.  Plain C++, no HIP: tests/fuzz/pair_plan.cc compiles it on the host under
// the sanitizers and checks every plan against a brute-force model.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace impop {

// ---- Gram cells.  I_ij is additive over disjoint site ranges, so overlapping (sliding) windows share the Gram matrices of the
// elementary segments between the sorted window boundaries: every site is contracted once however many windows cover it, and a
// window is the sum of its consecutive segments (formed on the fly by the statistics kernels, SimBatch.seg_*).  Without overlap
// the cells are the windows themselves.
struct PairCell {
    uint64_t b, e;
};
struct PairPlan {
    std::vector<PairCell> cells;         // all Gram cells, in site order when segmented
    std::vector<uint32_t> first, count;  // window i = cells [first[i], first[i] + count[i])
    std::vector<uint64_t> ord;           // the order the chunks take the windows in (segmented: by first cell, empty windows last)
    bool segmented = false;              // cells are elementary segments shared by windows (else: cell i is window i)
};
constexpr uint64_t PAIR_PLAN_MAX = 0xFFFFFFF0ull;  // cells and windows are counted in 32 bits

// windows: anything with site_begin / site_end, in the matrix's coordinates.  false: too many windows for a plan.
template <typename Win>
bool plan_cells(const Win *mw, uint64_t n_windows, PairPlan &p) {
    std::vector<PairCell> &cells = p.cells;
    std::vector<uint32_t> &first = p.first, &count = p.count;
    cells.clear();
    first.assign(n_windows, 0);
    count.assign(n_windows, 0);
    p.ord.resize(n_windows);
    for (uint64_t i = 0; i < n_windows; ++i) p.ord[i] = i;
    p.segmented = false;
    auto cells_are_windows = [&] {
        cells.resize(n_windows);
        for (uint64_t i = 0; i < n_windows; ++i) {
            cells[i] = {mw[i].site_begin, mw[i].site_end};
            first[i] = (uint32_t)i;
            count[i] = 1;
        }
    };
    // the usual window list — a BED tiling: sorted, no two windows overlapping — has nothing to share: its cells are the windows
    // (one O(n) check instead of the sort + searches below, 0.15 ms of host time per 4096 windows while the GPU waits)
    bool tiling = n_windows < PAIR_PLAN_MAX;
    for (uint64_t i = 1; i < n_windows && tiling; ++i) tiling = mw[i].site_begin >= mw[i - 1].site_end && mw[i].site_end >= mw[i].site_begin;
    if (tiling) {
        cells_are_windows();
        return true;
    }
    std::vector<uint64_t> cuts;
    uint64_t win_sites = 0;
    for (uint64_t i = 0; i < n_windows; ++i)
        if (mw[i].site_end > mw[i].site_begin) {
            cuts.push_back(mw[i].site_begin);
            cuts.push_back(mw[i].site_end);
            win_sites += mw[i].site_end - mw[i].site_begin;
        }
    std::sort(cuts.begin(), cuts.end());
    cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
    auto at = [&](uint64_t s) { return (size_t)(std::lower_bound(cuts.begin(), cuts.end(), s) - cuts.begin()); };
    std::vector<int64_t> cover(cuts.size() + 1, 0);
    for (uint64_t i = 0; i < n_windows; ++i)
        if (mw[i].site_end > mw[i].site_begin) {
            cover[at(mw[i].site_begin)] += 1;
            cover[at(mw[i].site_end)] -= 1;
        }
    std::vector<uint32_t> seg_before(cuts.size() + 1, 0);  // covered intervals left of cut k
    uint64_t seg_sites = 0;
    int64_t depth = 0;
    std::vector<PairCell> segs;
    for (size_t k = 0; k + 1 < cuts.size(); ++k) {
        seg_before[k] = (uint32_t)segs.size();
        depth += cover[k];
        if (depth > 0) {
            segs.push_back({cuts[k], cuts[k + 1]});
            seg_sites += cuts[k + 1] - cuts[k];
        }
    }
    if (!cuts.empty()) seg_before[cuts.size() - 1] = (uint32_t)segs.size();
    if (seg_sites * 20 < win_sites * 19 && segs.size() < PAIR_PLAN_MAX) {  // >= 5 % of the contraction is shared
        cells.swap(segs);
        p.segmented = true;
        for (uint64_t i = 0; i < n_windows; ++i)
            if (mw[i].site_end > mw[i].site_begin) {
                first[i] = seg_before[at(mw[i].site_begin)];
                count[i] = seg_before[at(mw[i].site_end)] - first[i];
            }
        std::stable_sort(p.ord.begin(), p.ord.end(), [&](uint64_t a, uint64_t b) {
            const bool ea = count[a] == 0, eb = count[b] == 0;  // empty windows last
            return ea != eb ? eb : (!ea && first[a] < first[b]);
        });
        return true;
    }
    if (n_windows >= PAIR_PLAN_MAX) return false;
    cells_are_windows();
    return true;
}

// ---- Chunks of consecutive (in `ord`) windows: at most win_cap windows whose cells span at most cap Gram matrices.
struct PairChunkSpan {
    uint64_t base = 0, cnt = 0;      // windows ord[base .. base + cnt)
    uint32_t c_lo = 0, n_cells = 0;  // their cells: [c_lo, c_lo + n_cells)
    // window wdx of this chunk starts at this Gram matrix of the chunk
    uint32_t first_of(const PairPlan &p, uint64_t wdx) const { return p.count[wdx] ? p.first[wdx] - c_lo : 0; }
    // problem k IS Gram matrix k (disjoint windows): the epilogue kernels then take their one-matrix variants
    bool one_to_one(const PairPlan &p) const {
        for (uint64_t k = 0; k < cnt; ++k)
            if (p.count[p.ord[base + k]] != 1 || first_of(p, p.ord[base + k]) != k) return false;
        return true;
    }
};
struct PairChunkWalk {
    enum Step { CHUNK, DONE, TOO_WIDE };
    const PairPlan &p;
    uint64_t cap, win_cap, cell_limit, base = 0;
    uint64_t bad_window = 0;  // TOO_WIDE: this window alone spans bad_cells > cap cells
    uint32_t bad_cells = 0;
    PairChunkWalk(const PairPlan &plan, uint64_t cap_, uint64_t win_cap_) : p(plan), cap(cap_), win_cap(win_cap_), cell_limit(cap_) {
        // even out the chunks: a total slightly above the capacity would otherwise leave a last chunk of a few
        // windows whose single-workgroup epilogue kernels cost their full latency
        if (p.cells.size() > cap) {
            uint32_t widest = 1;
            for (uint32_t c : p.count) widest = std::max(widest, c);
            uint64_t n_chunks = (p.cells.size() + cap - 1) / cap;
            if ((p.cells.size() + n_chunks - 1) / n_chunks + widest > cap) ++n_chunks;  // neighbours re-contract up to `widest` cells
            cell_limit = std::min<uint64_t>(cap, (p.cells.size() + n_chunks - 1) / n_chunks + widest);
        }
    }
    Step next(PairChunkSpan &c) {
        const uint64_t n_windows = p.ord.size();
        if (base >= n_windows) return DONE;
        uint64_t cnt = 0;
        uint32_t c_lo = 0, c_hi = 0;
        bool have = false;
        while (base + cnt < n_windows && cnt < cell_limit && cnt < win_cap) {
            const uint64_t wdx = p.ord[base + cnt];
            if (p.count[wdx]) {
                const uint32_t lo = have ? std::min(c_lo, p.first[wdx]) : p.first[wdx];
                const uint32_t hi = have ? std::max(c_hi, p.first[wdx] + p.count[wdx]) : p.first[wdx] + p.count[wdx];
                if ((uint64_t)(hi - lo) > (cnt == 0 ? cap : cell_limit)) {
                    if (cnt == 0) {
                        bad_window = wdx;
                        bad_cells = p.count[wdx];
                        return TOO_WIDE;
                    }
                    break;
                }
                c_lo = lo; c_hi = hi; have = true;
            }
            ++cnt;
        }
        c.base = base; c.cnt = cnt; c.c_lo = c_lo; c.n_cells = have ? c_hi - c_lo : 0;
        base += cnt;
        return CHUNK;
    }
};

}  // namespace impop
