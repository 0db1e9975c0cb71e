// paint_math.h — the arithmetic of impop_paint_scan (plain C++, no HIP types: tests/fuzz/paint_math.cc compiles it on the host under
// the sanitizers; paint.hip's kernels run the same functions on the device and define none of them).
// A state is one admissible donor of one recipient, numbered by its SLOT = its rank among the recipient's admissible donors in
// ascending haplotype order.  The device keeps, per state, R = V - (the minimum it last subtracted) in 32 bits and T = the site at
// which the state's current segment began; the cost M(L-1) is the 64-bit sum of the subtracted minima.
//   paint_site_update   the one-site update of a state: stay_j(s) = (R <= c_s) (a tie stays), T = s where it does not stay,
//                       R = mu [x_i(s) != x_j(s)] + min(R, c_s).  With R = V_j(s-1) - M(s-1) this is V_j(s) - M(s-1), which lies in
//                       0 .. c_s + mu <= 2^20 + 65535 < 2^21.  Site 0 is the same update from R = 0 with c_0 = 0.
//   paint_pack          (R, slot) in one 32-bit word, R in the upper 21 bits (22 with the idle value): the minimum of the words of
//                       all states is the minimum R, and among equal R the lowest slot = the lowest admissible haplotype, A(s).
//                       PAINT_IDLE is the R of a slot that holds no donor: above every real R, and its word still fits 32 bits.
//   paint_renorm        R -= the site's minimum, after it was added to the 64-bit cost: R stays below 2^21 for any number of sites.
//   paint_backtrack     the path from the per-site record (A(s), T(s) = the T of state A(s) after site s): the last segment is
//                       A(L-1) from T(L-1); the one before it ends at T(L-1) and is read at site T(L-1) - 1; one jump per segment.
//   paint_overlap       the sites of a segment [s0, s1) inside a window's stored-site range [w0, w1).
#pragma once
#include <stdint.h>

#include "dip_runs.h"  // DIP_HD

#define PAINT_FN DIP_HD inline __attribute__((always_inline))

namespace impop {

constexpr uint32_t PAINT_MAX_DONORS = 1024;      // IMPOP_PAINT_MAX_DONORS
constexpr uint32_t PAINT_MAX_RECIPIENTS = 4096;  // IMPOP_PAINT_MAX_RECIPIENTS
constexpr uint32_t PAINT_MAX_PANELS = 8;         // IMPOP_PAINT_MAX_PANELS
constexpr uint32_t PAINT_MAX_COST = 1048576;     // IMPOP_PAINT_MAX_COST
constexpr uint32_t PAINT_MAX_MU = 65535;
constexpr uint32_t PAINT_SLOT_BITS = 10;
constexpr uint32_t PAINT_IDLE = (1u << 22) - 1u;  // > PAINT_MAX_COST + PAINT_MAX_MU; (PAINT_IDLE << 10 | 1023) = 2^32 - 1
static_assert(PAINT_MAX_DONORS == 1u << PAINT_SLOT_BITS && PAINT_MAX_COST + PAINT_MAX_MU < PAINT_IDLE, "a packed word holds any state");

struct PaintRec {  // per site of a recipient
    uint32_t slot;  // A(s)
    uint32_t org;   // T(s): the site where the segment of state A(s) began
};

PAINT_FN void paint_site_update(uint32_t &R, uint32_t &T, uint32_t c, uint32_t mismatch, uint32_t mu, uint32_t s) {
    const bool stay = R <= c;
    T = stay ? T : s;
    R = (stay ? R : c) + (mismatch ? mu : 0u);
}

PAINT_FN uint32_t paint_pack(uint32_t R, uint32_t slot) { return (R << PAINT_SLOT_BITS) | slot; }
PAINT_FN uint32_t paint_pack_value(uint32_t w) { return w >> PAINT_SLOT_BITS; }
PAINT_FN uint32_t paint_pack_slot(uint32_t w) { return w & (PAINT_MAX_DONORS - 1u); }

PAINT_FN void paint_renorm(uint32_t &R, uint32_t site_min) { R -= site_min; }

// Calls seg(k, slot, s0, s1) for the segments from the LAST (k = 0) to the first, at most max_segments times (the host's bound on
// the loop); returns the number of segments, or max_segments + 1 where the bound ran out before site 0 was reached.
template <typename F>
PAINT_FN uint32_t paint_backtrack(const PaintRec *rec, uint32_t L, uint32_t max_segments, F seg) {
    uint32_t end = L, k = 0;
    while (end > 0) {
        if (k == max_segments) return max_segments + 1u;
        const PaintRec r = rec[end - 1];
        const uint32_t begin = r.org < end ? r.org : end - 1u;  // a record is never trusted to move the walk forwards
        seg(k, r.slot, begin, end);
        ++k;
        end = begin;
    }
    return k;
}

PAINT_FN uint32_t paint_overlap(uint32_t s0, uint32_t s1, uint32_t w0, uint32_t w1) {
    const uint32_t lo = s0 > w0 ? s0 : w0, hi = s1 < w1 ? s1 : w1;
    return hi > lo ? hi - lo : 0u;
}

}  // namespace impop
