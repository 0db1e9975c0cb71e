// ibs_plan.h — the host logic of impop_ibs_scan (plain C++, no HIP types: tests/fuzz/ibs_plan.cc compiles it on the host; ibs.hip
// runs the DIP_HD parts on the device): pair enumeration and pair tiles, the chunk / sub-segment cutter, the per-pair segment
// offsets with the pair ranges of one segment staging, and the window-edge accumulation.
//
// A pair's differing sites are folded into a DipSummary (dip_runs.h) per sub-segment; the summaries of consecutive stretches
// are joined with dip_combine.  With E = the join of everything left of a stretch, a difference at p closes the tract
// [E.het ? E.last + 1 : b, p); the tract behind the last difference is closed by the range's end.  The number of reported tracts
// closed so far follows from E alone (ibs_closed_before), so every tract knows its slot in the pair's part of the segment list.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "dip_runs.h"

namespace impop {

constexpr uint32_t IBS_TILE = 16;   // rows per side of an all-pairs tile: 256 pairs, one per thread; 32 rows' words = one LDS bank row
constexpr uint32_t IBS_PAIRS = IBS_TILE * IBS_TILE;
constexpr uint32_t IBS_BATCH = 32;  // 64-site blocks staged in LDS per barrier pair (8 KiB)

// index of the pair of member positions i < j among n members, i-major
DIP_HD inline uint64_t ibs_pair_index(uint32_t n, uint32_t i, uint32_t j) {
    return (uint64_t)i * (2ull * n - i - 1ull) / 2ull + (uint64_t)(j - i - 1u);
}

// reported tracts that the differences of E have closed: its inner runs and the leading one [b, E.first)
DIP_HD inline uint32_t ibs_closed_before(const DipSummary &E, uint64_t b, uint32_t min_sites) {
    return E.roh_runs + ((E.het != 0 && E.first - b >= min_sites) ? 1u : 0u);
}

// A tile of pairs, the work of one workgroup.  All-pairs form: the 16 member positions from 16 a0 x the 16 from 16 b0, a0 <= b0
// (a diagonal tile holds the pairs i < j only).  List form: pairs [256 a0, 256 a0 + 256) of the list.
struct IbsTile {
    uint32_t a0, b0;
};

// the tiles whose lowest .. highest pair index meets [p0, p1), in (a0, b0) order: every tile that holds a pair of the range, and
// near its ends a few that do not (a tile's pair indices are not contiguous; the lanes test their own pair)
inline std::vector<IbsTile> ibs_tiles_all(uint32_t n, uint64_t p0, uint64_t p1) {
    std::vector<IbsTile> t;
    if (n < 2 || p0 >= p1) return t;
    const uint32_t nb = (n + IBS_TILE - 1) / IBS_TILE;
    for (uint32_t a0 = 0; a0 < nb; ++a0) {
        const uint32_t a_first = a0 * IBS_TILE, a_end = std::min(n - 1, a_first + IBS_TILE);  // rows with a partner: i <= n - 2
        if (a_first >= a_end) continue;
        for (uint32_t b0 = a0; b0 < nb; ++b0) {
            const uint32_t b_first = std::max(b0 * IBS_TILE, a_first + 1), b_last = std::min(n, (b0 + 1) * IBS_TILE) - 1;
            if (b_first > b_last) continue;
            const uint32_t a_last = std::min(a_end - 1, b_last - 1);
            const uint64_t lo = ibs_pair_index(n, a_first, b_first), hi = ibs_pair_index(n, a_last, b_last);
            if (hi >= p0 && lo < p1) t.push_back(IbsTile{a0, b0});
        }
    }
    return t;
}
inline std::vector<IbsTile> ibs_tiles_list(uint64_t p0, uint64_t p1) {
    std::vector<IbsTile> t;
    if (p0 >= p1) return t;
    for (uint64_t k = p0 / IBS_PAIRS; k * IBS_PAIRS < p1; ++k) t.push_back(IbsTile{(uint32_t)k, 0u});
    return t;
}

// The cut of the range's n_blk 64-site blocks: chunks of chunk_blocks (one transposed buffer each), every chunk in sub-segments
// of seg_blocks that run in parallel.
struct IbsCut {
    uint64_t chunk_blocks = 1, seg_blocks = 1;
    uint64_t n_chunks = 0;
    uint32_t n_sub = 1;  // sub-segments of a full chunk
    uint64_t chunk_begin(uint64_t c) const { return c * chunk_blocks; }
    uint64_t chunk_len(uint64_t c, uint64_t n_blk) const { return std::min(chunk_blocks, n_blk - c * chunk_blocks); }
    uint32_t subs_of(uint64_t len) const { return (uint32_t)((len + seg_blocks - 1) / seg_blocks); }
};
constexpr uint64_t IBS_SUM_BYTES = 512ull << 20;  // the per-(sub-segment, pair) summaries of a chunk stay below this
constexpr uint32_t IBS_MAX_SUB = 65535;           // a grid's y extent

// words_budget: bytes the transposed words of a chunk may take (stride rows x 8 bytes per block).  env_chunk / env_seg: the test
// aids IMPOP_IBS_CHUNK_BLOCKS / IMPOP_IBS_SEG_BLOCKS (0: not set).  n_tiles workgroups per sub-segment; the default sub-segment
// length aims at 8 workgroups per compute unit, but at no fewer than IBS_BATCH blocks per sub-segment.
inline IbsCut ibs_cut(uint64_t n_blk, uint32_t stride, uint64_t n_pairs, uint64_t n_tiles, uint32_t n_cu, uint64_t words_budget,
                      uint32_t env_chunk, uint32_t env_seg) {
    IbsCut c;
    const uint64_t per_blk = (uint64_t)(stride ? stride : 1) * 8ull;
    c.chunk_blocks = env_chunk ? env_chunk : std::max<uint64_t>(1, words_budget / per_blk);
    c.chunk_blocks = std::max<uint64_t>(1, std::min<uint64_t>(c.chunk_blocks, n_blk ? n_blk : 1));
    c.chunk_blocks = std::min<uint64_t>(c.chunk_blocks, 1ull << 28);  // the transposing grid: 4 blocks per workgroup
    const uint64_t sum_cap = std::max<uint64_t>(1, IBS_SUM_BYTES / (std::max<uint64_t>(n_pairs, 1) * sizeof(DipSummary)));
    uint64_t want = env_seg ? (c.chunk_blocks + env_seg - 1) / env_seg
                            : (8ull * (n_cu ? n_cu : 1) + std::max<uint64_t>(n_tiles, 1) - 1) / std::max<uint64_t>(n_tiles, 1);
    // by default no sub-segment shorter than one staged batch: the combine kernel walks a pair's sub-segments one after the other
    if (!env_seg) want = std::min<uint64_t>(want, (c.chunk_blocks + IBS_BATCH - 1) / IBS_BATCH);
    want = std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(want, c.chunk_blocks), std::min<uint64_t>(sum_cap, IBS_MAX_SUB)));
    c.seg_blocks = (c.chunk_blocks + want - 1) / want;
    c.n_sub = c.subs_of(c.chunk_blocks);
    c.n_chunks = (n_blk + c.chunk_blocks - 1) / c.chunk_blocks;
    return c;
}

// exclusive prefix of the pairs' tract counts: off[p] = the first segment of pair p, off[n] = the total
template <typename Count>
inline std::vector<uint64_t> ibs_offsets(uint64_t n_pairs, Count n_tracts_of) {
    std::vector<uint64_t> off(n_pairs + 1, 0);
    for (uint64_t p = 0; p < n_pairs; ++p) off[p + 1] = off[p] + n_tracts_of(p);
    return off;
}
// pair ranges [r[k], r[k + 1]) whose segments fit a staging of seg_cap records; a range always takes one pair
inline std::vector<uint64_t> ibs_pair_ranges(const std::vector<uint64_t> &off, uint64_t seg_cap) {
    std::vector<uint64_t> r{0};
    const uint64_t n = off.size() - 1;
    uint64_t p = 0;
    while (p < n) {
        uint64_t q = (uint64_t)(std::upper_bound(off.begin() + p, off.end(), off[p] + seg_cap) - off.begin()) - 1;  // off[q] <= off[p] + cap
        q = std::max(q, p + 1);
        r.push_back(std::min(q, n));
        p = r.back();
    }
    return r;
}

// ---- window records from the reported tracts, with no per-site array ----------------------------------------------------------
// edge: the windows' 2 n_windows edges, sorted, distinct.  For a tract [s, t): i0 = the first edge > s, i1 = the first edge >= t.
// Four difference arrays of n_edge + 1 entries: nA[i0] += 1, sA[i0] += s, nB[i1] += 1, tB[i1] += t.  Their prefixes at edge x:
//     A(x) = tracts with s < x      B(x) = tracts with t <= x      SA, TB likewise
//     C(x) = sum min(max(x - s, 0), t - s) = (A - B) x - SA + TB     (uint64 arithmetic, exact modulo 2^64)
// pair_sites of [wb, we) = C(we) - C(wb), tracts = A(we) - B(wb).  Containment is no function of single edges: the non-empty
// windows sorted by begin (sbeg, their ends send) — a tract looks at those that begin in [s, t) and counts into span[k] when
// send[k] <= t.  Every loop is bounded by the host's counts.
struct IbsWindowsDev {  // as the kernels see the tables
    const uint64_t *edge = nullptr, *sbeg = nullptr, *send = nullptr;
    unsigned long long *acc = nullptr;  // nA | sA | nB | tB, n_edge + 1 each, then span[n_span]
    uint32_t n_edge = 0, n_span = 0;
};
DIP_HD inline uint32_t ibs_first_above(const uint64_t *a, uint32_t n, uint64_t x, bool or_equal) {  // first k with a[k] > x (>= x)
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (or_equal ? a[mid] >= x : a[mid] > x) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}
template <typename Add>
DIP_HD inline void ibs_add_tract(const IbsWindowsDev &w, uint64_t s, uint64_t t, Add add) {
    const uint32_t i0 = ibs_first_above(w.edge, w.n_edge, s, false), i1 = ibs_first_above(w.edge, w.n_edge, t, true);
    const uint64_t stride = (uint64_t)w.n_edge + 1;
    add(w.acc + i0, 1ull);
    add(w.acc + stride + i0, (unsigned long long)s);
    add(w.acc + 2 * stride + i1, 1ull);
    add(w.acc + 3 * stride + i1, (unsigned long long)t);
    unsigned long long *span = w.acc + 4 * stride;
    const uint32_t k1 = ibs_first_above(w.sbeg, w.n_span, t, true);
    for (uint32_t k = ibs_first_above(w.sbeg, w.n_span, s, true); k < k1; ++k)
        if (w.send[k] <= t) add(span + k, 1ull);
}

struct IbsWindowSums {
    uint64_t pair_sites = 0, tracts = 0, spanning = 0;
};
struct IbsWindowPlan {
    std::vector<uint64_t> edge, sbeg, send;
    std::vector<uint32_t> ib, ie;    // per window: the indices of its two edges
    std::vector<int64_t> span_of;    // per window: its slot in the begin-sorted list, -1 for an empty window
    size_t acc_words() const { return 4 * (edge.size() + 1) + sbeg.size(); }
    // wb / we: the windows' edges
    void build(const uint64_t *wb, const uint64_t *we, uint64_t n) {
        edge.clear();
        for (uint64_t i = 0; i < n; ++i) {
            edge.push_back(wb[i]);
            edge.push_back(we[i]);
        }
        std::sort(edge.begin(), edge.end());
        edge.erase(std::unique(edge.begin(), edge.end()), edge.end());
        ib.resize(n);
        ie.resize(n);
        std::vector<uint64_t> order;
        for (uint64_t i = 0; i < n; ++i) {
            ib[i] = (uint32_t)(std::lower_bound(edge.begin(), edge.end(), wb[i]) - edge.begin());
            ie[i] = (uint32_t)(std::lower_bound(edge.begin(), edge.end(), we[i]) - edge.begin());
            if (we[i] > wb[i]) order.push_back(i);
        }
        std::stable_sort(order.begin(), order.end(), [&](uint64_t x, uint64_t y) { return wb[x] < wb[y]; });
        span_of.assign(n, -1);
        sbeg.resize(order.size());
        send.resize(order.size());
        for (size_t k = 0; k < order.size(); ++k) {
            sbeg[k] = wb[order[k]];
            send[k] = we[order[k]];
            span_of[order[k]] = (int64_t)k;
        }
    }
    // acc as the tracts left it -> the sums of every window
    std::vector<IbsWindowSums> finish(const unsigned long long *acc) const {
        const size_t ne = edge.size(), stride = ne + 1;
        std::vector<uint64_t> A(ne), B(ne), Cx(ne);
        uint64_t a = 0, sa = 0, b = 0, tb = 0;
        for (size_t i = 0; i < ne; ++i) {
            a += acc[i];
            sa += acc[stride + i];
            b += acc[2 * stride + i];
            tb += acc[3 * stride + i];
            A[i] = a;
            B[i] = b;
            Cx[i] = (a - b) * edge[i] - sa + tb;
        }
        std::vector<IbsWindowSums> out(ib.size());
        for (size_t i = 0; i < ib.size(); ++i) {
            if (span_of[i] < 0) continue;  // an empty window meets nothing
            out[i].pair_sites = Cx[ie[i]] - Cx[ib[i]];
            out[i].tracts = A[ie[i]] - B[ib[i]];
            out[i].spanning = acc[4 * stride + (size_t)span_of[i]];
        }
        return out;
    }
};

}  // namespace impop
