// ibd_chain.h — the rule of impop_ibd_scan (include/impop_hip.h) as plain C++ (no HIP types: tests/fuzz/ibd_chain.cc compiles it
// on the host; ibd.hip runs the DIP_HD parts on the device): the genetic map G, the classes of a tract, and the chain step.
//
// A pair's tracts come in ascending order, 64 at a time (one per lane of a wave).  Of a batch, cmask holds the lanes whose tract
// is a candidate, smask those that are seeds, bmask the candidates that do NOT join the candidate in front of them (the gap to
// it exceeds max_gap, or there is none): the heads of the chains.  A chain is then a head and the candidates up to the next
// head, all plain bit ranges (ibd_chain_lanes), and its sums are differences of a prefix sum over the lanes.  The candidates in
// front of the first head extend the chain the batches before left open (IbdChain, uniform over the wave); the last head's chain
// stays open.  ibd_chain_batch is that step written with explicit lanes, for the host; ibd_chain_kernel is the same step with
// ballots and shuffles.
#pragma once
#include <stdint.h>

#include "dip_runs.h"  // DIP_HD

namespace impop {

struct IbdMap {  // n == 0: G(x) = x
    const uint64_t *pos = nullptr, *g = nullptr;
    uint32_t n = 0;
};
struct IbdRule {
    uint64_t min_seed = 0, min_extend = 0, min_output = 0;  // units of G
    uint64_t max_gap = 0;                                     // coordinates
    uint32_t min_sites = 1;
};

// the map's steps are below 2^32 in pos and in g (ibd_map_check), so the product fits 64 bits.  At most 32 probes.
DIP_HD inline uint64_t ibd_map_eval(const IbdMap &m, uint64_t x) {
    if (m.n == 0) return x;
    if (x <= m.pos[0]) return m.g[0];
    if (x >= m.pos[m.n - 1]) return m.g[m.n - 1];
    uint32_t lo = 0, hi = m.n - 1;  // pos[lo] <= x < pos[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (m.pos[mid] <= x) lo = mid;
        else hi = mid;
    }
    return m.g[lo] + (x - m.pos[lo]) * (m.g[lo + 1] - m.g[lo]) / (m.pos[lo + 1] - m.pos[lo]);
}
// 0: the map is usable, else the index of the first breakpoint that is not (pos strictly ascending, g non-decreasing, steps < 2^32)
inline uint64_t ibd_map_check(const uint64_t *pos, const uint64_t *g, uint64_t n) {
    for (uint64_t k = 1; k < n; ++k)
        if (pos[k] <= pos[k - 1] || g[k] < g[k - 1] || pos[k] - pos[k - 1] >= (1ull << 32) || g[k] - g[k - 1] >= (1ull << 32)) return k;
    return 0;
}

constexpr uint32_t IBD_CANDIDATE = 1u, IBD_SEED = 2u;
// the class of a tract of `extent` sites and length `len`: 0, IBD_CANDIDATE, or IBD_CANDIDATE | IBD_SEED
DIP_HD inline uint32_t ibd_class(const IbdRule &r, uint64_t extent, uint64_t len) {
    if (extent < r.min_sites || len < r.min_extend) return 0u;
    return IBD_CANDIDATE | (len >= r.min_seed ? IBD_SEED : 0u);
}
// does a candidate that begins at s open a new chain?  prev_end: the end of the candidate in front of it, if there is one
DIP_HD inline bool ibd_breaks(bool has_prev, uint64_t prev_end, uint64_t s, uint64_t max_gap) { return !has_prev || s - prev_end > max_gap; }

struct IbdChain {
    uint64_t begin = 0, gbegin = 0, end = 0, gend = 0;  // the first candidate's begin, the last one's end, G at both
    uint32_t n = 0, sites = 0;                          // candidates and the sum of their extents
    uint32_t seed = 0, open = 0;
};
DIP_HD inline IbdChain ibd_chain_make(uint64_t begin, uint64_t gbegin, uint64_t end, uint64_t gend, uint32_t n, uint32_t sites, bool seed) {
    IbdChain c;
    c.begin = begin;
    c.gbegin = gbegin;
    c.end = end;
    c.gend = gend;
    c.n = n;
    c.sites = sites;
    c.seed = seed ? 1u : 0u;
    c.open = 1u;
    return c;
}
// n more candidates, the last ending at `end`, join the open chain
DIP_HD inline void ibd_chain_extend(IbdChain &c, uint64_t end, uint64_t gend, uint32_t n, uint32_t sites, bool seed) {
    c.end = end;
    c.gend = gend;
    c.n += n;
    c.sites += sites;
    c.seed |= seed ? 1u : 0u;
}
DIP_HD inline bool ibd_reported(const IbdChain &c, const IbdRule &r) { return c.open && c.seed && c.gend - c.gbegin >= r.min_output; }

// ---- the batch's lane masks ----
DIP_HD inline uint64_t ibd_lanes_below(uint32_t l) { return l >= 64 ? ~0ull : (1ull << l) - 1ull; }
DIP_HD inline uint32_t ibd_top_lane(uint64_t m) { return 63u - (uint32_t)__builtin_clzll(m); }  // m != 0
DIP_HD inline uint32_t ibd_low_lane(uint64_t m) { return m ? (uint32_t)__builtin_ctzll(m) : 64u; }
// the candidate in front of `lane` inside the batch, or -1
DIP_HD inline int ibd_prev_lane(uint64_t cmask, uint32_t lane) {
    const uint64_t m = cmask & ibd_lanes_below(lane);
    return m ? (int)ibd_top_lane(m) : -1;
}
// the candidates of the chain whose head is lane j: from j up to the next head
DIP_HD inline uint64_t ibd_chain_lanes(uint64_t cmask, uint64_t bmask, uint32_t j) {
    const uint32_t stop = ibd_low_lane(bmask & ~ibd_lanes_below(j + 1));
    return cmask & ibd_lanes_below(stop) & ~ibd_lanes_below(j);
}
// the candidates in front of the first head: they extend the chain left open
DIP_HD inline uint64_t ibd_head_lanes(uint64_t cmask, uint64_t bmask) { return cmask & ibd_lanes_below(ibd_low_lane(bmask)); }

// One batch of n <= 64 tracts [s[i], t[i]) of a pair, ascending, against the chain `c` that the batches before left open.
// emit(chain) receives every chain that closes inside the batch and is reported.  The host's form of ibd_chain_kernel's loop body.
template <typename Emit>
inline void ibd_chain_batch(IbdChain &c, const uint64_t *s, const uint64_t *t, uint32_t n, const IbdMap &map, const IbdRule &rule,
                            uint32_t *n_candidates, Emit emit) {
    uint64_t gs[64], gt[64], cmask = 0, smask = 0, bmask = 0;
    uint32_t ext[64], pre[64];
    for (uint32_t l = 0; l < n; ++l) {
        gs[l] = ibd_map_eval(map, s[l]);
        gt[l] = ibd_map_eval(map, t[l]);
        const uint32_t cls = ibd_class(rule, t[l] - s[l], gt[l] - gs[l]);
        if (cls & IBD_CANDIDATE) cmask |= 1ull << l;
        if (cls & IBD_SEED) smask |= 1ull << l;
        ext[l] = (cls & IBD_CANDIDATE) ? (uint32_t)(t[l] - s[l]) : 0u;
        pre[l] = ext[l] + (l ? pre[l - 1] : 0u);
    }
    for (uint32_t l = 0; l < n; ++l) {
        if (!((cmask >> l) & 1)) continue;
        const int pl = ibd_prev_lane(cmask, l);
        if (ibd_breaks(pl >= 0 || c.open, pl >= 0 ? t[pl] : c.end, s[l], rule.max_gap)) bmask |= 1ull << l;
    }
    *n_candidates += (uint32_t)__builtin_popcountll(cmask);
    const uint64_t head = ibd_head_lanes(cmask, bmask);
    if (head) {
        const uint32_t top = ibd_top_lane(head);
        ibd_chain_extend(c, t[top], gt[top], (uint32_t)__builtin_popcountll(head), pre[top], (smask & head) != 0);
    }
    if (!bmask) return;
    if (ibd_reported(c, rule)) emit(c);
    const uint32_t last = ibd_top_lane(bmask);
    for (uint32_t l = 0; l < n; ++l) {
        if (!((bmask >> l) & 1)) continue;
        const uint64_t lanes = ibd_chain_lanes(cmask, bmask, l);
        const uint32_t top = ibd_top_lane(lanes);
        const IbdChain mine = ibd_chain_make(s[l], gs[l], t[top], gt[top], (uint32_t)__builtin_popcountll(lanes), pre[top] - pre[l] + ext[l],
                                             (smask & lanes) != 0);
        if (l == last) c = mine;
        else if (ibd_reported(mine, rule)) emit(mine);
    }
}
// behind the pair's last batch
template <typename Emit>
inline void ibd_chain_finish(IbdChain &c, const IbdRule &rule, Emit emit) {
    if (ibd_reported(c, rule)) emit(c);
    c = IbdChain();
}

}  // namespace impop
