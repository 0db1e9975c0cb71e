// ihs_math.h — the integer arithmetic of impop_ihs_scan that the host and the device share (include/impop_hip.h has the
// definitions): the cutoff comparison, a break's nearest-greater spans and its share of an integral, reach and flag rules, the
// chunk -> block mapping and the warm-up start.  Plain C++, no HIP types: tests/fuzz/ihs_math.cc compiles it on the host under
// the sanitizers and checks every piece against a step-by-step model of its own.
//
// Steps.  A walk numbers the stepped sites it visits 0, 1, ... from its warm-up start in its own direction (dir 0 ascends the
// ordinals and fills half 0, the match towards lower coordinates; dir 1 descends and fills half 1).  After step s the PBWT
// holds, per neighbour in its order, d = the first step of their match into s (d = s + 1: they differ at s; a match that began
// before the warm-up start has d = 0).  A pair's match begins at the maximum of the d between its two positions.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define IHS_HD __host__ __device__ inline
#else
#define IHS_HD inline
#endif

namespace impop {

constexpr uint32_t IHS_GROUP = 32;  // spans skip whole groups of this many breaks by the groups' maxima

// the cutoff: does a class with C pairs, `surv` of them left, still count as homozygous
IHS_HD bool ihs_cut_ok(uint64_t surv, uint64_t C, uint32_t cutoff_milli) { return 1000ull * surv >= (uint64_t)cutoff_milli * C; }

// Break t of the breaks [lo, hi) (d(i) = divergence at i, gmax(g) = max of d over [32 g, 32 g + 32), consulted only for groups
// that lie wholly inside [lo, hi)) is the maximum of exactly left * right position pairs: `left` counts t and the breaks below
// it that are smaller (strict), `right` t and the breaks above it that are not larger.  Every pair is owned by its leftmost maximum.
template <typename D, typename GM>
IHS_HD uint32_t ihs_span_left(uint32_t t, uint32_t lo, uint32_t hi, D d, GM gmax) {
    const uint32_t v = d(t);
    uint32_t i = t;  // i: the lowest break known to belong to the span
    while (i > lo) {
        if ((i & (IHS_GROUP - 1)) == 0 && i - lo >= IHS_GROUP && i <= hi && gmax((i >> 5) - 1) < v) {
            i -= IHS_GROUP;
            continue;
        }
        if (d(i - 1) >= v) break;
        --i;
    }
    return t - i + 1;
}
template <typename D, typename GM>
IHS_HD uint32_t ihs_span_right(uint32_t t, uint32_t lo, uint32_t hi, D d, GM gmax) {
    const uint32_t v = d(t);
    uint32_t i = t;  // i: the highest break known to belong to the span
    while (i + 1 < hi) {
        if (((i + 1) & (IHS_GROUP - 1)) == 0 && hi - (i + 1) >= IHS_GROUP && i + 1 >= lo && gmax((i + 1) >> 5) <= v) {
            i += IHS_GROUP;
            continue;
        }
        if (d(i + 1) > v) break;
        ++i;
    }
    return i - t + 1;
}

// What the w pairs whose match begins at step d add to twice the trapezoid integral of a core at step s that stops at step
// x_end < d: (U(d) + U(d - 1)) each, U = distance from the core.  Pairs that differ at the core itself (d = s + 1) add nothing.
IHS_HD uint64_t ihs_break_term(uint64_t w, uint32_t d, uint32_t s, uint64_t U_d, uint64_t U_dm1) { return d > s ? 0ull : w * (U_d + U_dm1); }
// and the pairs still alive at x_end: the full distance, twice
IHS_HD uint64_t ihs_alive_term(uint64_t surv_end, uint64_t U_end) { return surv_end * 2ull * U_end; }

// first index in [0, n) with pos(i) >= v (n when none)
template <typename P>
IHS_HD uint64_t ihs_lower_bound(P pos, uint64_t n, uint64_t v) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (pos(mid) < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The farthest stepped ordinal a walk from ordinal x may reach in direction dir under one measure's limit (measure 0: base
// pairs, |p - p(x)| <= limit; measure 1: sites, |ordinal - x| <= limit; limit 0: none), n_st stepped sites, pos(i) ascending.
template <typename P>
IHS_HD uint64_t ihs_far(int dir, int measure, uint64_t x, uint64_t n_st, uint64_t limit, P pos) {
    const uint64_t edge = dir ? n_st - 1 : 0;
    if (!limit) return edge;
    if (measure == 1) return dir ? (n_st - 1 - x > limit ? x + limit : edge) : (x > limit ? x - limit : edge);
    const uint64_t p = pos(x);
    if (!dir) return p > limit ? ihs_lower_bound(pos, x, p - limit) : edge;  // pos(x) itself qualifies: the result is <= x
    const uint64_t top = p + limit < p ? ~0ull : p + limit;
    if (top == ~0ull) return edge;
    return ihs_lower_bound(pos, n_st, top + 1) - 1;  // >= x
}
// The same for the next core of a walk, from the previous core's answer: reaches are monotone along a walk, so the pointer only
// moves the walk's way and all cores of a chunk together cost one pass over the positions.  prev = the reach of an earlier core.
template <typename P>
IHS_HD uint64_t ihs_far_advance(int dir, uint64_t prev, uint64_t x, uint64_t n_st, uint64_t limit, P pos) {
    if (!limit) return dir ? n_st - 1 : 0;
    const uint64_t p = pos(x);
    uint64_t f = prev;
    if (!dir) {
        while (f < x && p - pos(f) > limit) ++f;
    } else {
        while (f > x && pos(f) - p > limit) --f;
    }
    return f;
}
// the range's own end: nothing beyond it exists.  A reach that ends there is an EDGE, every other reach a LIMIT.
IHS_HD bool ihs_far_is_edge(int dir, uint64_t far, uint64_t n_st) { return far == (dir ? n_st - 1 : 0); }

// flag bits of one (measure, class, half): bit 4 measure + 2 class + half, EDGE in the low byte and LIMIT in the next
IHS_HD uint32_t ihs_flag(int measure, int cls, int half, bool at_reach, bool edge) {
    if (!at_reach) return 0u;
    return 1u << ((edge ? 0 : 8) + 4 * measure + 2 * cls + half);
}

// Chunks: the range's blocks [0, n_blk) in runs of chunk_blocks.
struct IhsChunks {
    uint64_t n_blk = 0, chunk_blocks = 1;
    IHS_HD uint64_t count() const { return (n_blk + chunk_blocks - 1) / chunk_blocks; }
    IHS_HD uint64_t begin(uint64_t c) const { return c * chunk_blocks; }
    IHS_HD uint64_t end(uint64_t c) const { return (c + 1) * chunk_blocks < n_blk ? (c + 1) * chunk_blocks : n_blk; }
};
// The default chunk length: a chunk steps 8 times its expected warm-up, so that the warm-up is a minor share, but no more than
// gives every compute unit two chunks per direction (the work at the cores outweighs the steps, and it only spreads over chunks),
// and at least 1024 stepped sites.  A measure without a limit warms up from the range's end: one chunk is the only sensible cut.
inline IhsChunks ihs_chunks(uint64_t n_blk, uint64_t n_st, uint64_t range_bp, uint64_t max_bp, uint64_t max_sites, uint32_t forced_blocks,
                            uint32_t n_cu) {
    IhsChunks c;
    c.n_blk = n_blk;
    c.chunk_blocks = n_blk ? n_blk : 1;
    if (forced_blocks) c.chunk_blocks = forced_blocks;
    else if (max_bp && max_sites && n_st && n_blk) {
        // expected warm-up steps: the tighter of the two limits decides nothing, the looser one does
        const long double per_bp = (long double)n_st / (long double)(range_bp ? range_bp : 1);
        const long double by_bp = per_bp * (long double)max_bp;
        uint64_t warm = by_bp > (long double)n_st ? n_st : (uint64_t)by_bp;
        if (max_sites > warm) warm = max_sites < n_st ? max_sites : n_st;
        uint64_t steps = warm * 8;
        const uint64_t spread = n_st / (2ull * (n_cu ? n_cu : 1));
        if (steps > spread) steps = spread;
        if (steps < 1024) steps = 1024;
        const uint64_t per_blk = (n_st + n_blk - 1) / n_blk;  // >= 1
        c.chunk_blocks = (steps + per_blk - 1) / per_blk;
    }
    if (c.chunk_blocks < 1) c.chunk_blocks = 1;
    if (c.chunk_blocks > c.n_blk && c.n_blk) c.chunk_blocks = c.n_blk;
    return c;
}

// The warm-up start of a chunk whose stepped ordinals are [o0, o1), o0 < o1: the farthest ordinal either measure lets the
// chunk's first stepped site (in walk order) reach.  No core of the chunk reaches farther, because reaches are monotone.
template <typename P>
IHS_HD uint64_t ihs_warm_start(int dir, uint64_t o0, uint64_t o1, uint64_t n_st, uint64_t max_bp, uint64_t max_sites, P pos) {
    const uint64_t x = dir ? o1 - 1 : o0;
    const uint64_t a = ihs_far(dir, 0, x, n_st, max_bp, pos), b = ihs_far(dir, 1, x, n_st, max_sites, pos);
    return dir ? (a > b ? a : b) : (a < b ? a : b);
}

}  // namespace impop
