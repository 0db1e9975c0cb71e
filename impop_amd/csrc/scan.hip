// scan.hip — the HBM-bound hot path: one streaming pass over the SB64 presence matrix gives,
// per window, S, sum c(n-c) for the subset P and populations A, B, the A x B cross sum, and
// from those pi, Hudson Fst and Tajima's D.
//
// Work decomposition: windows -> elementary segments (so overlapping / sliding windows read
// every site once) -> tiles of <= tile_blocks 64-site blocks.  One 256-thread workgroup per
// tile; wave w takes blocks b0+w, b0+w+4, ...; lane l of a wave owns site 64b+l and pulls its
// wps dwords with ceil(wps/4) fully coalesced 1 KiB wave loads (layout: internal.h).  The
// three population masks are wave-uniform and live in SGPRs.  Integer partials per tile are
// written once (no atomics => deterministic); a second tiny kernel sums each window's tiles
// and evaluates the fp64 statistics in the reference's operation order.  Plans of many small tiles on a unique-row route run
// the second body instead, one WAVE per tile and four tiles per workgroup (scan_tiles_kernel_wave) — and, where the plan is kept
// for more launches, read a per-tile digest of everything no mask enters, built where the plan is made (scan_tiles_kernel_digest).
#include <algorithm>
#include <map>
#include <vector>

#include "device_utils.h"
#include "hap_words.h"
#include "internal.h"
#include "pop_stream.h"
#include "sb64.h"
#include "scan_route.h"
#include "tile_digest.h"

namespace impop {

struct TilePartial {  // 48 B
    uint32_t s_all, s_p, s_a, s_b;
    uint64_t sum_p, sum_a, sum_b, sum_ab;
};
struct PopSizes {
    uint32_t n, nP, nA, nB;
};

template <int WPS>
struct MaskArgs {
    uint32_t p[WPS], a[WPS], b[WPS];
};

// Tuning knobs (defaults chosen by tools/tune_scan.py on MI355X; IMPOP_SCAN_NT: sb64.h)
// Measured (tools/tune_scan.py, 465 x 75 M sites, interleaved rounds): unroll / occupancy / tile
// size move the result by < 2 % once nt is on; a 64-VGPR cap (min_waves 8 at unroll 2) spills.
#ifndef IMPOP_SCAN_UNROLL
#define IMPOP_SCAN_UNROLL 0    // 64-site blocks in flight per wave; 0 = auto (about 8 wave loads in flight)
#endif
#ifndef IMPOP_SCAN_MIN_WAVES
#define IMPOP_SCAN_MIN_WAVES 6 // __launch_bounds__ 2nd argument (waves per SIMD)
#endif

// per-lane sums of one tile, any n <= 65535: every product c (n - c) is below 2^32, the sums are 64 bits wide
struct LaneAcc {
    typedef uint64_t sum_t;
    static __device__ __forceinline__ uint32_t mul(uint32_t a, uint32_t b) { return a * b; }
    uint32_t s_all = 0, s_p = 0, s_a = 0, s_b = 0;
    uint64_t q_p = 0, q_a = 0, q_b = 0, q_ab = 0;
};

// Fixed-WPS kernel (n <= 512): every product c (n - c) is below 2^16, so the lane accumulators of one
// tile fit 32 bits (<= 1024 sites per lane and tile) and the multiply is a 24-bit v_mul / v_mad
// (v_mul_lo_u32 is a quarter-rate instruction); they are widened once, at the tile reduction.  This is
// what lifts the small-n cases, which are VALU-bound rather than HBM-bound (4-16 B per site).
struct LaneAcc32 {
    typedef uint32_t sum_t;
    static __device__ __forceinline__ uint32_t mul(uint32_t a, uint32_t b) { return __umul24(a, b); }
    uint32_t s_all = 0, s_p = 0, s_a = 0, s_b = 0;
    uint32_t q_p = 0, q_a = 0, q_b = 0, q_ab = 0;
};

// One site per lane, wt = its weight.  No validity test here: lanes outside the tile had their words zeroed by the caller
// (only the first / last block of a tile can be partial), and all-zero words add nothing to any counter.
// Segregating test 0 < c < n as ONE unsigned compare: (c - 1) < (n - 1)  (false for n = 0 or 1 as well).
template <bool SUBSET_P, typename Acc>
__device__ __forceinline__ void counts_accumulate(uint32_t c, uint32_t cP, uint32_t cA, uint32_t cB, const PopSizes &ps, Acc &acc,
                                                  typename Acc::sum_t wt = 1) {
    typedef typename Acc::sum_t sum_t;
    if (!SUBSET_P) cP = c;
    acc.s_all += (c - 1u) < (ps.n - 1u);
    acc.s_p += (cP - 1u) < (ps.nP - 1u);
    acc.s_a += (cA - 1u) < (ps.nA - 1u);
    acc.s_b += (cB - 1u) < (ps.nB - 1u);
    const uint32_t rA = ps.nA - cA, rB = ps.nB - cB;
    acc.q_p += wt * Acc::mul(cP, ps.nP - cP);
    acc.q_a += wt * Acc::mul(cA, rA);
    acc.q_b += wt * Acc::mul(cB, rB);
    acc.q_ab += wt * ((sum_t)Acc::mul(cA, rB) + (sum_t)Acc::mul(cB, rA));
}

// A representative of the distinct-row stream (internal.h, d_vuniq): its counts stand for wt rows, equal or complemented, and
// every term is linear in wt — s_x += wt [segregating], q_x += wt product — and the same for a row and its complement (c <-> n - c
// in every population at once: 0 < c < n, c (n - c) and cA (nB - cB) + cB (nA - cA) stay).  wt <= 64 and every product is
// at most 2^16 (the cross term: nA nB with nA + nB <= 512), so each wt x product is a 24-bit multiply; the lane sums: tile_cut.h, UNIQ_MID_MAX.
template <bool SUBSET_P>
__device__ __forceinline__ void counts_accumulate_folded(uint32_t c, uint32_t cP, uint32_t cA, uint32_t cB, const PopSizes &ps,
                                                         LaneAcc32 &acc, uint32_t wt) {
    if (!SUBSET_P) cP = c;
    acc.s_all += (c - 1u) < (ps.n - 1u) ? wt : 0u;
    acc.s_p += (cP - 1u) < (ps.nP - 1u) ? wt : 0u;
    acc.s_a += (cA - 1u) < (ps.nA - 1u) ? wt : 0u;
    acc.s_b += (cB - 1u) < (ps.nB - 1u) ? wt : 0u;
    const uint32_t rA = ps.nA - cA, rB = ps.nB - cB;
    acc.q_p += __umul24(wt, __umul24(cP, ps.nP - cP));
    acc.q_a += __umul24(wt, __umul24(cA, rA));
    acc.q_b += __umul24(wt, __umul24(cB, rB));
    acc.q_ab += __umul24(wt, __umul24(cA, rB) + __umul24(cB, rA));
}

// FOLDED: the row is a representative of weight wt (counts_accumulate_folded), else a row of its own
template <int WPS, bool SUBSET_P, bool FOLDED = false>
__device__ __forceinline__ void site_accumulate(const uint32_t (&w)[WPS], const MaskArgs<WPS> &mk, const PopSizes &ps,
                                                LaneAcc32 &acc, uint32_t wt = 1) {
    uint32_t c = 0, cP = 0, cA = 0, cB = 0;
#pragma unroll
    for (int k = 0; k < WPS; ++k) {
        c += __popc(w[k]);
        if (SUBSET_P) cP += __popc(w[k] & mk.p[k]);
        cA += __popc(w[k] & mk.a[k]);
        cB += __popc(w[k] & mk.b[k]);
    }
    if constexpr (FOLDED) counts_accumulate_folded<SUBSET_P>(c, cP, cA, cB, ps, acc, wt);
    else counts_accumulate<SUBSET_P>(c, cP, cA, cB, ps, acc);
}

// rare_listed_in (hap_words.h): how many of the haplotypes a rare entry lists belong to a population
// ... and the counts of the 1-allele follow, mirrored through n - m, nP - mP, ... when the listed haplotypes carry 0 (then
// every 0-carrier is listed).  Exact integers as for a row.  One loop over the slots tests all three masks (not three calls of
// rare_listed_in): most sites of the headline workload arrive here, and three separate loops measured 4 % slower there.
template <bool SUBSET_P>
__device__ __forceinline__ void rare_counts(uint64_t v, const uint32_t *lp, const uint32_t *la, const uint32_t *lb, const PopSizes &ps,
                                            uint32_t &c, uint32_t &cP, uint32_t &cA, uint32_t &cB) {
    const uint32_t m = rare_count(v);
    uint32_t mP = 0, mA = 0, mB = 0;
#pragma unroll
    for (uint32_t i = 0; i < IMPOP_RARE_MAX; ++i)
        if (i < m) {
            const uint32_t h = rare_slot(v, i), wd = h >> 5, bit = h & 31u;
            mA += (la[wd] >> bit) & 1u;
            mB += (lb[wd] >> bit) & 1u;
            if (SUBSET_P) mP += (lp[wd] >> bit) & 1u;
        }
    if (rare_lists_zeros(v)) { c = ps.n - m; cP = ps.nP - mP; cA = ps.nA - mA; cB = ps.nB - mB; }
    else { c = m; cP = mP; cA = mA; cB = mB; }
}

// The fixed-WPS kernel (n <= 512) decodes an entry through a table in LDS instead: hcode[h] holds, in three 5-bit fields, whether
// haplotype h belongs to A, B and P (bit 15: to both A and B, for single_range), and entry RARE_CODE_NONE is 0, where the unused
// slots of an entry (0xFFFF) land.  The sum of
// an entry's three table values is (mA, mB, mP), its listed haplotypes per population, in three bit-field reads, three LDS reads
// and one add — no per-slot predicate, no 64-bit shifts.
// Which allele the listed haplotypes carry does not matter here: with c = m or n - m alike, c (n - c) = m (n - m), the cross
// term cA (nB - cB) + cB (nA - cA) = mA (nB - mB) + mB (nA - mA), and 0 < c < n iff 0 < m < n.  So the tile's sums follow from
// the moments sum m, sum m^2 and sum mA mB, folded once per lane and tile (RareMoments::fold): exact integers, the same totals.
constexpr uint32_t RARE_CODE_SIZE = 1024, RARE_CODE_NONE = RARE_CODE_SIZE - 1;  // > 512 haplotypes; 0xFFFF & 1023 = 1023
struct RareMoments {
    uint32_t a1 = 0, b1 = 0, p1 = 0, a2 = 0, b2 = 0, p2 = 0, ab = 0;
    __device__ __forceinline__ void add(uint64_t e, const uint16_t *hcode, const PopSizes &ps, LaneAcc32 &acc) {
        const uint32_t lo = (uint32_t)e, hi = (uint32_t)(e >> 32);
        const uint32_t code = (uint32_t)hcode[(lo >> 16) & RARE_CODE_NONE] + (uint32_t)hcode[hi & RARE_CODE_NONE] +
                              (uint32_t)hcode[(hi >> 16) & RARE_CODE_NONE];
        const uint32_t m = rare_count(e), mA = code & 31u, mB = (code >> 5) & 31u, mP = (code >> 10) & 31u;
        acc.s_all += (m - 1u) < (ps.n - 1u);
        acc.s_p += (mP - 1u) < (ps.nP - 1u);
        acc.s_a += (mA - 1u) < (ps.nA - 1u);
        acc.s_b += (mB - 1u) < (ps.nB - 1u);
        a1 += mA; b1 += mB; p1 += mP;
        a2 += __umul24(mA, mA); b2 += __umul24(mB, mB); p2 += __umul24(mP, mP); ab += __umul24(mA, mB);
    }
    // sum m (n - m) = n sum m - sum m^2;  sum [mA (nB - mB) + mB (nA - mA)] = nB sum mA + nA sum mB - 2 sum mA mB
    __device__ __forceinline__ void fold(const PopSizes &ps, LaneAcc32 &acc) const {
        acc.q_p += ps.nP * p1 - p2;
        acc.q_a += ps.nA * a1 - a2;
        acc.q_b += ps.nB * b1 - b2;
        acc.q_ab += ps.nB * a1 + ps.nA * b1 - 2u * ab;
    }
};
// NT threads share the entries [e0, e1), tid = this thread's index among them: the workgroup's 256, or the 64 of a one-wave tile
template <int NT = 256>
__device__ __forceinline__ void rare_range_coded(const uint64_t *__restrict__ rare, uint64_t e0, uint64_t e1, const uint16_t *hcode,
                                                 const PopSizes &ps, LaneAcc32 &acc, uint32_t tid) {
    constexpr int RU = 4;
    RareMoments mo;
    uint64_t e = e0 + tid;
    for (; e + NT * (RU - 1) < e1; e += NT * RU) {
        uint64_t v[RU];
#pragma unroll
        for (int u = 0; u < RU; ++u) v[u] = stream_load(rare + e + NT * u);
#pragma unroll
        for (int u = 0; u < RU; ++u) mo.add(v[u], hcode, ps, acc);
    }
    for (; e < e1; e += NT) mo.add(stream_load(rare + e), hcode, ps, acc);
    mo.fold(ps, acc);
}

// What a lane's singletons add to its sums, from how many there are (k) and how many of their carriers lie in A, in B, in P and in
// both A and B: RareMoments::fold at m = 1.  single_range and the tile digest's histogram (scan_tiles_kernel_digest) close with it.
__device__ __forceinline__ void singles_fold(uint32_t k, uint32_t kA, uint32_t kB, uint32_t kP, uint32_t kAB, const PopSizes &ps,
                                             LaneAcc32 &acc) {
    acc.s_all += k;
    acc.s_p += ps.nP > 1u ? kP : 0u;
    acc.s_a += ps.nA > 1u ? kA : 0u;
    acc.s_b += ps.nB > 1u ? kB : 0u;
    acc.q_p += kP * (ps.nP - 1u);
    acc.q_a += kA * (ps.nA - 1u);
    acc.q_b += kB * (ps.nB - 1u);
    acc.q_ab += ps.nB * kA + ps.nA * kB - 2u * kAB;
}

// The packed route's singleton stream (internal.h, d_vsingle): singletons [s0, s1) of a tile, 2 bytes each, read as the aligned
// 8-byte words [s0 / 4, ceil(s1 / 4)) — thread t takes word w0 + t, w0 + t + 256, ..., SU of them in flight (non-temporal,
// 512 bytes per wave load; the stream's 0xFFFF padding keeps the last word inside the allocation).  Slots outside [s0, s1) —
// only the first and the last word have any — are set to 0xFFFF, which the table maps to RARE_CODE_NONE like an unused slot of
// an entry.  A singleton has m = 1, so every per-population count is 0 or 1 and the tile's sums follow from how many of its
// singletons' carriers lie in A, in B, in P and in both A and B (bit 15 of a table value; the plan removes that overlap, the
// kernel does not rely on it): per word four table reads and three adds, per batch of SU words one unpack of the four fields
// (a 5-bit field holds the 4 * SU = 16 a batch can add), and once per lane and tile
//     S: s_all += k, s_x += kX when nX > 1;   sum m (nX - m) = kX (nX - 1);   cross = nB kA + nA kB - 2 kAB   (RareMoments::fold at m = 1)
// Exact integers, the same totals as the 8-byte entries give.  The 32-bit lane accumulators still hold: the tile budget counts 8
// bytes per rare site whichever stream it sits in, so a tile has at most tile_blocks x 64 x 4 WPS / 8 <= 2^21 rare sites at
// tile_blocks = 4096, 2^13 per lane, each adding at most 2 x 511 to a sum — below 2^24 next to the rows' 2^27.
// SKIP (the instantiations with the distinct-row stream): a word past the range in every lane of the wave is not decoded (a
// ballot): four table reads that add nothing — a bench tile holds 2.2 words per thread where a batch decodes SU = 4
// NT, tid as in rare_range_coded; SU words in flight per thread, 4 SU <= 31 for the 5-bit fields.  A one-wave tile (NT = 64)
// takes SU = 5: the 550 words of a bench tile are two batches, 9 words decoded per lane and one skipped
template <bool SKIP = false, int NT = 256, int SU = 4>
__device__ __forceinline__ void single_range(const uint16_t *__restrict__ single, uint64_t s0, uint64_t s1, const uint16_t *hcode,
                                             const PopSizes &ps, LaneAcc32 &acc, uint32_t tid) {
    static_assert(4 * SU <= 31, "a batch overflows a 5-bit field of the table's sums");
    const uint64_t *words = reinterpret_cast<const uint64_t *>(single);
    const uint64_t w0 = s0 >> 2, w1 = (s1 + 3) >> 2;
    const uint32_t head = (uint32_t)(s0 & 3), tail = (uint32_t)(s1 & 3);  // slots cut off the first word, slots kept of the last (0: all)
    uint32_t k = 0, kA = 0, kB = 0, kP = 0, kAB = 0;
    for (uint64_t w = w0 + tid; w < w1; w += NT * SU) {
        uint64_t v[SU];
#pragma unroll
        for (int u = 0; u < SU; ++u) {
            const uint64_t i = w + NT * u;
            v[u] = stream_load(words + (i < w1 ? i : w1 - 1));  // past the range: a word of it again, dropped below
        }
        uint32_t code = 0;
#pragma unroll
        for (int u = 0; u < SU; ++u) {
            const uint64_t i = w + NT * u;
            if constexpr (SKIP) {
                if (__builtin_amdgcn_ballot_w64(i < w1) == 0) continue;
            }
            uint64_t x = i < w1 ? v[u] : ~0ull;
            uint32_t in = i < w1 ? 4u : 0u;
            if (i == w0 && head) { x |= (1ull << (16 * head)) - 1ull; in -= head; }
            if (i == w1 - 1 && tail) { x |= ~0ull << (16 * tail); in -= 4u - tail; }
            const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
            code += (uint32_t)hcode[lo & RARE_CODE_NONE] + (uint32_t)hcode[(lo >> 16) & RARE_CODE_NONE] +
                    (uint32_t)hcode[hi & RARE_CODE_NONE] + (uint32_t)hcode[(hi >> 16) & RARE_CODE_NONE];
            k += in;
        }
        kA += code & 31u; kB += (code >> 5) & 31u; kP += (code >> 10) & 31u; kAB += code >> 15;
    }
    singles_fold(k, kA, kB, kP, kAB, ps, acc);
}

// entries [e0, e1) of a tile, thread t takes e0 + t, e0 + t + 256, ...: RU coalesced 512-byte wave loads in flight per wave
template <bool SUBSET_P, typename Acc>
__device__ __forceinline__ void rare_range(const uint64_t *__restrict__ rare, uint64_t e0, uint64_t e1, const uint32_t *lp,
                                           const uint32_t *la, const uint32_t *lb, const PopSizes &ps, Acc &acc) {
    constexpr int RU = 4;
    uint64_t e = e0 + threadIdx.x;
    for (; e + 256 * (RU - 1) < e1; e += 256 * RU) {
        uint64_t v[RU];
#pragma unroll
        for (int u = 0; u < RU; ++u) v[u] = stream_load(rare + e + 256 * u);
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            uint32_t c, cP, cA, cB;
            rare_counts<SUBSET_P>(v[u], lp, la, lb, ps, c, cP, cA, cB);
            counts_accumulate<SUBSET_P>(c, cP, cA, cB, ps, acc);
        }
    }
    for (; e < e1; e += 256) {
        uint32_t c, cP, cA, cB;
        rare_counts<SUBSET_P>(stream_load(rare + e), lp, la, lb, ps, c, cP, cA, cB);
        counts_accumulate<SUBSET_P>(c, cP, cA, cB, ps, acc);
    }
}

__device__ __forceinline__ void tile_reduce_store(LaneAcc &acc, TilePartial *out) {
    __shared__ uint64_t red[4][8];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t s0 = wave_sum_u32(acc.s_all), s1 = wave_sum_u32(acc.s_p), s2 = wave_sum_u32(acc.s_a),
                   s3 = wave_sum_u32(acc.s_b);
    const uint64_t q0 = wave_sum_u64(acc.q_p), q1 = wave_sum_u64(acc.q_a), q2 = wave_sum_u64(acc.q_b),
                   q3 = wave_sum_u64(acc.q_ab);
    if (lane == 0) {
        red[wave][0] = s0; red[wave][1] = s1; red[wave][2] = s2; red[wave][3] = s3;
        red[wave][4] = q0; red[wave][5] = q1; red[wave][6] = q2; red[wave][7] = q3;
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        const uint64_t v = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
        TilePartial *o = out + blockIdx.x;
        switch (threadIdx.x) {
            case 0: o->s_all = (uint32_t)v; break;
            case 1: o->s_p = (uint32_t)v; break;
            case 2: o->s_a = (uint32_t)v; break;
            case 3: o->s_b = (uint32_t)v; break;
            case 4: o->sum_p = v; break;
            case 5: o->sum_a = v; break;
            case 6: o->sum_b = v; break;
            default: o->sum_ab = v; break;
        }
    }
}

// The same store from 32-bit lane sums, the wave sums taken in the VALU (wave_sum_u32_dpp): the 72 ds_bpermute of a wave in
// tile_reduce_store are LDS instructions, and a workgroup that moves 20 KB is short of LDS issue slots before it is short of
// anything else.  A lane sum is below 2^32 and 64 of them are not: each is summed as its low and its
// high 16 bits, two wave sums below 2^22.
__device__ __forceinline__ void tile_reduce_store32(const LaneAcc32 &acc, TilePartial *out) {
    __shared__ uint64_t red[4][8];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    auto wide = [](uint32_t q) { return (uint64_t)wave_sum_u32_dpp(q & 0xFFFFu) + ((uint64_t)wave_sum_u32_dpp(q >> 16) << 16); };
    const uint32_t s0 = wave_sum_u32_dpp(acc.s_all), s1 = wave_sum_u32_dpp(acc.s_p), s2 = wave_sum_u32_dpp(acc.s_a),
                   s3 = wave_sum_u32_dpp(acc.s_b);
    const uint64_t q0 = wide(acc.q_p), q1 = wide(acc.q_a), q2 = wide(acc.q_b), q3 = wide(acc.q_ab);
    if (lane == 63) {
        red[wave][0] = s0; red[wave][1] = s1; red[wave][2] = s2; red[wave][3] = s3;
        red[wave][4] = q0; red[wave][5] = q1; red[wave][6] = q2; red[wave][7] = q3;
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        const uint64_t v = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
        TilePartial *o = out + blockIdx.x;
        switch (threadIdx.x) {
            case 0: o->s_all = (uint32_t)v; break;
            case 1: o->s_p = (uint32_t)v; break;
            case 2: o->s_a = (uint32_t)v; break;
            case 3: o->s_b = (uint32_t)v; break;
            case 4: o->sum_p = v; break;
            case 5: o->sum_a = v; break;
            case 6: o->sum_b = v; break;
            default: o->sum_ab = v; break;
        }
    }
}

// Rows [s0, s1) of an SB64 base, one of the up to three row ranges of a tile: blocks [s0 / 64, ceil(s1 / 64)), U of them per
// iteration (U*ceil(WPS/4) independent 1 KiB wave loads in flight per wave).  Only the first and the last block of a range can be
// partial: lanes before s0 in the first and from s1 on in the last get all-zero words (wave-uniform branch, taken for those two
// blocks only); interior blocks carry no validity arithmetic and no branch, so all U loads of an iteration are in flight together.
// FOLDED: the base is the distinct-row stream and wts its weight bytes, one per row, loaded with the row.
// turn: the tile's ranges hand their blocks to the four waves from ONE running block index (a bench tile is a head block, one or
// two blocks of representatives and a tail block: three loops that each start at wave 0 would give all of them to one wave and
// serialise the loads).  In: how many blocks of this range go by before this wave's first; out: the same for the next range.
// NW: the waves that share the range, 4 or the 1 of a one-wave tile (turn stays 0).
template <int WPS, bool SUBSET_P, bool FOLDED, int U, int NW = 4>
__device__ __forceinline__ void row_range(const uint32_t *__restrict__ sb, const uint8_t *__restrict__ wts, uint64_t s0, uint64_t s1,
                                          uint32_t &turn, uint32_t lane, const MaskArgs<WPS> &mk, const PopSizes &ps, LaneAcc32 &acc) {
    if (s1 <= s0) return;  // uniform over the NW waves
    const uint64_t b0 = s0 >> 6, b1 = (s1 + 63) >> 6;
    const uint32_t lo = (uint32_t)(s0 - (b0 << 6));
    const uint32_t hi = (uint32_t)(s1 - ((b1 - 1) << 6));  // 1..64
    auto trim = [&](uint32_t (&w)[WPS], uint64_t blk) {
        if ((blk == b0 && lo != 0) | (blk == b1 - 1 && hi != 64)) {
            const bool keep = lane >= (blk == b0 ? lo : 0u) && lane < (blk == b1 - 1 ? hi : 64u);
#pragma unroll
            for (int k = 0; k < WPS; ++k) w[k] = keep ? w[k] : 0u;
        }
    };
    uint64_t b = b0 + turn;
    turn = (turn + (uint32_t)NW - (uint32_t)((b1 - b0) & (NW - 1))) & (uint32_t)(NW - 1);
    for (; b + NW * (U - 1) < b1; b += NW * U) {
        uint32_t w[U][WPS], wt[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            load_site<WPS>(sb + (b + NW * u) * (64ull * WPS), lane, w[u]);
            wt[u] = FOLDED ? (uint32_t)stream_load(wts + (b + NW * u) * 64 + lane) : 1u;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            trim(w[u], b + NW * u);
            site_accumulate<WPS, SUBSET_P, FOLDED>(w[u], mk, ps, acc, wt[u]);
        }
    }
    if constexpr (U > 1) {
        for (; b < b1; b += NW) {
            uint32_t w0[WPS];
            load_site<WPS>(sb + b * (64ull * WPS), lane, w0);
            const uint32_t wt0 = FOLDED ? (uint32_t)stream_load(wts + b * 64 + lane) : 1u;
            trim(w0, b);
            site_accumulate<WPS, SUBSET_P, FOLDED>(w0, mk, ps, acc, wt0);
        }
    }
}

// uniqs (unique-row route, else null): the tile's range of the distinct-row stream, indexed like the tile.  Not empty: the tile's
// whole blocks of rows are read as their representatives (uniq, uniq_wt) and only its head and its tail, the partial blocks at
// window edges (tile_cut.h, mid_blocks), as rows of sb.  Empty: every row of the tile from sb.
// UNIQ: the plan's route has the stream.  A plan without it launches the instantiation without: one row range and none of the
// stream's arguments in registers — the kernel it was before the stream (the weighted range and the third range cost
// <15,false> six SGPRs and with them a wave of occupancy, 8 -> 7, which a route that reads no representative need not pay).
template <int WPS, bool SUBSET_P, bool UNIQ>
__global__ __launch_bounds__(256, IMPOP_SCAN_MIN_WAVES) void scan_tiles_kernel(const uint32_t *__restrict__ sb,
                                                                               const uint64_t *__restrict__ rare,
                                                                               const ScanTile *__restrict__ tiles,
                                                                               const MaskArgs<WPS> mk, const PopSizes ps,
                                                                               TilePartial *__restrict__ out,
                                                                               const uint16_t *__restrict__ single,
                                                                               const SingleRange *__restrict__ singles,
                                                                               const uint32_t *__restrict__ uniq,
                                                                               const uint8_t *__restrict__ uniq_wt,
                                                                               const UniqRange *__restrict__ uniqs) {
    const ScanTile t = tiles[blockIdx.x];
    // packed route: the tile's range of the singleton stream (null otherwise), indexed like the tile — no dependent load
    SingleRange sr = {0, 0};
    if (singles) sr = singles[blockIdx.x];
    UniqRange ur = {0, 0};
    if constexpr (UNIQ) ur = uniqs[blockIdx.x];
    const TileBlocks tb = tile_blocks_of(t);
    // split index: this thread's share of the haplotype code table (RareMoments) — the mask words of haplotypes threadIdx.x and
    // threadIdx.x + 256, read from the kernel arguments (MaskArgs is p | a | b) BEFORE the rows so that they arrive behind them
    constexpr int CODE_PER_THREAD = (32 * WPS + 255) / 256;
    const bool has_single = sr.end > sr.begin;                            // workgroup-uniform, as the next
    const bool has_rare = t.rare_end > t.rare_begin || has_single;        // the table is needed
    uint32_t mw[CODE_PER_THREAD][3] = {};
    if (has_rare) {
        const uint32_t *mkw = reinterpret_cast<const uint32_t *>(&mk);
#pragma unroll
        for (int j = 0; j < CODE_PER_THREAD; ++j) {
            const uint32_t h = threadIdx.x + 256u * j;
            if (h < 32u * WPS) { mw[j][0] = mkw[h >> 5]; mw[j][1] = mkw[WPS + (h >> 5)]; mw[j][2] = mkw[2 * WPS + (h >> 5)]; }
        }
    }
    LaneAcc32 acc;
    constexpr int G = (WPS + 3) / 4;
    constexpr int U = IMPOP_SCAN_UNROLL > 0 ? IMPOP_SCAN_UNROLL : (G >= 3 ? 2 : G == 2 ? 4 : 8);
    // head | whole blocks as representatives | tail; without a range the head is the whole tile
    if constexpr (UNIQ) {
        uint32_t turn = tb.wave;
        const bool folded = ur.end > ur.begin;  // workgroup-uniform
        const MidBlocks mid = mid_blocks(t.site_begin, t.site_end);
        const uint64_t head_end = folded ? mid.g0 << 6 : t.site_end, tail_begin = folded ? mid.g1 << 6 : t.site_end;
        row_range<WPS, SUBSET_P, false, U>(sb, nullptr, t.site_begin, head_end, turn, tb.lane, mk, ps, acc);
        row_range<WPS, SUBSET_P, true, U>(uniq, uniq_wt, ur.begin, ur.end, turn, tb.lane, mk, ps, acc);
        row_range<WPS, SUBSET_P, false, 1>(sb, nullptr, tail_begin, t.site_end, turn, tb.lane, mk, ps, acc);  // one block at most
    } else {
        // the tile's blocks tb.b0 .. tb.b1, wave w taking b0 + w, b0 + w + 4, ...: row_range over the whole tile, written out so
        // that this instantiation stays the kernel it was, register for register
        uint64_t b = tb.b0 + tb.wave;
        const uint32_t lo = (uint32_t)(t.site_begin - (tb.b0 << 6));
        const uint32_t hi = (uint32_t)(t.site_end - ((tb.b1 - 1) << 6));  // 1..64
        auto trim = [&](uint32_t (&w)[WPS], uint64_t blk) {
            if ((blk == tb.b0 && lo != 0) | (blk == tb.b1 - 1 && hi != 64)) {
                const bool keep = tb.lane >= (blk == tb.b0 ? lo : 0u) && tb.lane < (blk == tb.b1 - 1 ? hi : 64u);
#pragma unroll
                for (int k = 0; k < WPS; ++k) w[k] = keep ? w[k] : 0u;
            }
        };
        for (; b + 4 * (U - 1) < tb.b1; b += 4 * U) {
            uint32_t w[U][WPS];
#pragma unroll
            for (int u = 0; u < U; ++u) load_site<WPS>(sb + (b + 4 * u) * (64ull * WPS), tb.lane, w[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                trim(w[u], b + 4 * u);
                site_accumulate<WPS, SUBSET_P>(w[u], mk, ps, acc);
            }
        }
        for (; b < tb.b1; b += 4) {
            uint32_t w0[WPS];
            load_site<WPS>(sb + b * (64ull * WPS), tb.lane, w0);
            trim(w0, b);
            site_accumulate<WPS, SUBSET_P>(w0, mk, ps, acc);
        }
    }
    if (has_rare) {
        __shared__ uint16_t hcode[RARE_CODE_SIZE];
#pragma unroll
        for (int j = 0; j < CODE_PER_THREAD; ++j) {
            const uint32_t h = threadIdx.x + 256u * j, bit = h & 31u;
            if (h < 32u * WPS)
                hcode[h] = (uint16_t)(((mw[j][1] >> bit) & 1u) | (((mw[j][2] >> bit) & 1u) << 5) | (((mw[j][0] >> bit) & 1u) << 10) |
                                      (((mw[j][1] & mw[j][2]) >> bit & 1u) << 15));
        }
        if (threadIdx.x == 0) hcode[RARE_CODE_NONE] = 0;
        __syncthreads();
        rare_range_coded(rare, t.rare_begin, t.rare_end, hcode, ps, acc, threadIdx.x);
        if (has_single) single_range<UNIQ>(single, sr.begin, sr.end, hcode, ps, acc, threadIdx.x);
    }
    if constexpr (UNIQ) {
        tile_reduce_store32(acc, out);
    } else {
        LaneAcc wide;
        wide.s_all = acc.s_all; wide.s_p = acc.s_p; wide.s_a = acc.s_a; wide.s_b = acc.s_b;
        wide.q_p = acc.q_p; wide.q_a = acc.q_a; wide.q_b = acc.q_b; wide.q_ab = acc.q_ab;
        tile_reduce_store(wide, out);
    }
}

// The 48-byte partial of a one-wave tile: no LDS and no barrier, the wave sums in the VALU (lanes 48..63 hold them) and lane 63
// writes the record itself.  A lane sum is below 2^32 by the plan's cap (tile_cut.h, wave_tile_fits), summed as two halves as above.
__device__ __forceinline__ void wave_reduce_store32(const LaneAcc32 &acc, uint32_t lane, TilePartial *o) {
    auto wide = [](uint32_t q) { return (uint64_t)wave_sum_u32_dpp(q & 0xFFFFu) + ((uint64_t)wave_sum_u32_dpp(q >> 16) << 16); };
    TilePartial r;
    r.s_all = wave_sum_u32_dpp(acc.s_all); r.s_p = wave_sum_u32_dpp(acc.s_p); r.s_a = wave_sum_u32_dpp(acc.s_a);
    r.s_b = wave_sum_u32_dpp(acc.s_b);
    r.sum_p = wide(acc.q_p); r.sum_a = wide(acc.q_a); r.sum_b = wide(acc.q_b); r.sum_ab = wide(acc.q_ab);
    if (lane == 63) *o = r;
}

// The code table of a workgroup whose waves own a tile each, filled by all 256 threads from the masks in the kernel arguments
// (the caller's barrier follows): set_masks acts at the next launch.
template <int WPS>
__device__ __forceinline__ void code_table_fill(uint16_t *hcode, const MaskArgs<WPS> &mk) {
    constexpr int CODE_PER_THREAD = (32 * WPS + 255) / 256;
    const uint32_t *mkw = reinterpret_cast<const uint32_t *>(&mk);  // p | a | b
#pragma unroll
    for (int j = 0; j < CODE_PER_THREAD; ++j) {
        const uint32_t h = threadIdx.x + 256u * j, bit = h & 31u;
        if (h < 32u * WPS) {
            const uint32_t mp = mkw[h >> 5], ma = mkw[WPS + (h >> 5)], mb = mkw[2 * WPS + (h >> 5)];
            hcode[h] = (uint16_t)(((ma >> bit) & 1u) | (((mb >> bit) & 1u) << 5) | (((mp >> bit) & 1u) << 10) |
                                  (((ma & mb) >> bit & 1u) << 15));
        }
    }
    if (threadIdx.x == 0) hcode[RARE_CODE_NONE] = 0;
}

// The second body of the fixed-WPS kernel on a unique-row route: ONE WAVE PER TILE, wave w of workgroup g owns tile 4 g + w.
// A bench tile is about 20 KB — a head block, one or two blocks of representatives, a tail block, some 46 entries and 2 200
// singletons — so in scan_tiles_kernel each of the four waves owns at most one block, and everything else a wave executes (tile
// decode, the dispatch around three row ranges, the table share, entries, singletons, 72 DPP adds, the store) is per-wave fixed
// cost that all four pay for the same tile: the kernel is bound by VALU issue of that replicated overhead (DESIGN.md 4.1, round
// 25).  Here a tile pays it once.  The wave index is scalar, so the tile, its SingleRange and its UniqRange come through scalar
// loads and every per-tile branch is a scalar branch; the ranges are the same row_range, rare_range_coded and single_range at
// stride 1 block / 64 threads.  The code table is filled once per workgroup by all 256 threads — the four tiles share the plan's
// masks — whatever the tiles hold (whether a tile has rare sites is not workgroup-uniform here), and that barrier is the only
// one: after it the four waves never meet again, and a wave past the last tile leaves.  Which plans run this body: tile_cut.h,
// wave_tile_choice — the 32-bit lane sums hold four times as much of a tile as in the four-wave body.
template <int WPS, bool SUBSET_P>
__global__ __launch_bounds__(256, 5) void scan_tiles_kernel_wave(const uint32_t *__restrict__ sb, const uint64_t *__restrict__ rare,
                                                                 const ScanTile *__restrict__ tiles, const MaskArgs<WPS> mk,
                                                                 const PopSizes ps, TilePartial *__restrict__ out,
                                                                 const uint16_t *__restrict__ single,
                                                                 const SingleRange *__restrict__ singles,
                                                                 const uint32_t *__restrict__ uniq, const uint8_t *__restrict__ uniq_wt,
                                                                 const UniqRange *__restrict__ uniqs, uint32_t n_tiles) {
    __shared__ uint16_t hcode[RARE_CODE_SIZE];
    code_table_fill<WPS>(hcode, mk);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t k = 4u * blockIdx.x + (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // scalar
    if (k >= n_tiles) return;
    const ScanTile t = tiles[k];
    SingleRange sr = {0, 0};
    if (singles) sr = singles[k];
    const UniqRange ur = uniqs[k];
    LaneAcc32 acc;
    constexpr int G = (WPS + 3) / 4;
    constexpr int U = IMPOP_SCAN_UNROLL > 0 ? IMPOP_SCAN_UNROLL : (G >= 3 ? 2 : G == 2 ? 4 : 8);
    uint32_t turn = 0;
    const bool folded = ur.end > ur.begin;
    const MidBlocks mid = mid_blocks(t.site_begin, t.site_end);
    const uint64_t head_end = folded ? mid.g0 << 6 : t.site_end, tail_begin = folded ? mid.g1 << 6 : t.site_end;
    row_range<WPS, SUBSET_P, false, U, 1>(sb, nullptr, t.site_begin, head_end, turn, lane, mk, ps, acc);
    row_range<WPS, SUBSET_P, true, U, 1>(uniq, uniq_wt, ur.begin, ur.end, turn, lane, mk, ps, acc);
    row_range<WPS, SUBSET_P, false, 1, 1>(sb, nullptr, tail_begin, t.site_end, turn, lane, mk, ps, acc);  // one block at most
    if (t.rare_end > t.rare_begin) rare_range_coded<64>(rare, t.rare_begin, t.rare_end, hcode, ps, acc, lane);
    if (sr.end > sr.begin) single_range<true, 64, 5>(single, sr.begin, sr.end, hcode, ps, acc, lane);
    wave_reduce_store32(acc, lane, out + k);
}

// The one-wave body on a plan with a tile digest (tile_digest.h; built where the plan is made, digest_build_kernel below): the
// same workgroup — wave w of workgroup g owns tile 4 g + w, one table, one barrier — and the same TilePartial, from what the
// plan worked out once because no mask enters it.  A tile's common rows are ONE run of weighted representatives (a bench tile:
// about 29 of them, one block, where the body above walks a head, one or two blocks of the stream and a tail through three
// dispatches), with neither trim nor range arithmetic: a lane at or past the count loads nothing and accumulates zero words at
// weight 0.  Its singletons are 32 WPS uint16 counts: lane l reads those of haplotypes 8 l .. 8 l + 7 in one 16-byte load and
// their table values in one LDS read, eight multiplies by table bits in place of nine decoded words.  A tile whose range of the
// singleton stream is shorter than a histogram kept it (a scalar branch).  The entries are the rare stream's, as above.
// The digest is read again at every launch and is a fraction of the plan's streams, so its loads are plain ones (the
// streams' are non-temporal: read once).
template <int WPS, bool SUBSET_P>
__global__ __launch_bounds__(256, 5) void scan_tiles_kernel_digest(const uint32_t *__restrict__ rows, const uint16_t *__restrict__ wts,
                                                                   const uint16_t *__restrict__ hists,
                                                                   const DigestDesc *__restrict__ descs,
                                                                   const uint64_t *__restrict__ rare,
                                                                   const uint16_t *__restrict__ single, const MaskArgs<WPS> mk,
                                                                   const PopSizes ps, TilePartial *__restrict__ out, uint32_t n_tiles) {
    __shared__ __attribute__((aligned(16))) uint16_t hcode[RARE_CODE_SIZE];
    code_table_fill<WPS>(hcode, mk);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t k = 4u * blockIdx.x + (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // scalar
    if (k >= n_tiles) return;
    const DigestDesc d = descs[k];
    // the histogram's 16 bytes go out first and arrive behind the rows; lanes past the 32 WPS haplotypes hold no count
    u32v4 cnt = {0u, 0u, 0u, 0u};
    if (d.hist != 0 && lane < 4u * WPS) cnt = *reinterpret_cast<const u32v4 *>(hists + ((uint64_t)(d.hist - 1) * (32u * WPS) + 8u * lane));
    LaneAcc32 acc;
    const uint32_t padded = (uint32_t)digest_rows_padded(d.n_rows);
    const uint32_t *base = rows + d.row_off * WPS;
    for (uint32_t b = 0; b < d.n_rows; b += 64) {
        const uint32_t i = b + lane;
        uint32_t w[WPS] = {}, wt = 0;
        if (i < d.n_rows) {
            load_row<WPS, false>(base, padded, i, w);
            wt = wts[d.row_off + i];
        }
        site_accumulate<WPS, SUBSET_P, true>(w, mk, ps, acc, wt);
    }
    if (d.rare_end > d.rare_begin) rare_range_coded<64>(rare, d.rare_begin, d.rare_end, hcode, ps, acc, lane);
    if (d.hist != 0) {
        // table values past 32 WPS are unset and meet a count of 0
        const u32v4 code = *reinterpret_cast<const u32v4 *>(hcode + 8u * lane);
        uint32_t n1 = 0, kA = 0, kB = 0, kP = 0, kAB = 0;
        auto add = [&](uint32_t c, uint32_t v) {
            n1 += c;
            kA += __umul24(c, v & 1u); kB += __umul24(c, (v >> 5) & 1u); kP += __umul24(c, (v >> 10) & 1u); kAB += __umul24(c, (v >> 15) & 1u);
        };
        const uint32_t cw[4] = {cnt.x, cnt.y, cnt.z, cnt.w}, vw[4] = {code.x, code.y, code.z, code.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            add(cw[j] & 0xFFFFu, vw[j] & 0xFFFFu);
            add(cw[j] >> 16, vw[j] >> 16);
        }
        singles_fold(n1, kA, kB, kP, kAB, ps, acc);
    } else if (d.single_end > d.single_begin) {
        single_range<true, 64, 5>(single, d.single_begin, d.single_end, hcode, ps, acc, lane);
    }
    wave_reduce_store32(acc, lane, out + k);
}

// Any wps (n > 512 haplotypes, and every weighted matrix): the three masks of the WHOLE haplotype axis sit in
// LDS (3 x wps dwords, <= 24 KB at the 65 535-haplotype limit; filled once per workgroup) and come back as
// broadcast ds_read_b128 — every lane the same address, no bank conflict — so a wave simply streams the
// granules of one 64-site block after the other, AN_U fully coalesced 1 KiB loads in flight, with the four
// per-site counts in registers for the length of the block.  Every byte of the tile is read exactly once.
// (Round 1 walked the haplotype axis in 16-dword chunks whose masks were re-loaded into SGPRs per chunk for up
// to 8 blocks per wave: 6.08 TB/s on the 4096 x 10^7 launch, and tiles were pinned to 32 blocks = 1 MB, which
// left a fifth of the chip idle in the last wave of tiles.)
// WEIGHTED (impop_matrix_set_site_weights): column s stands for w_s base pairs (a graph node of that length), so
// every sum_s c (n - c) becomes sum_s w_s c (n - c) and the window's W is sum_s w_s (host prefix sums at plan
// time) — exactly what scanning the bp-expanded matrix gives — while the segregating-site counts stay counts
// of COLUMNS (variable nodes, what a VCF of the window lists).
constexpr int AN_U = 8;  // granules (1 KiB wave loads) in flight per wave

template <bool SUBSET_P>
__device__ __forceinline__ void anyn_granule(const u32v4 v, const uint32_t *lp, const uint32_t *la, const uint32_t *lb,
                                             uint32_t g, uint32_t &c, uint32_t &cP, uint32_t &cA, uint32_t &cB) {
    const u32v4 ka = *reinterpret_cast<const u32v4 *>(la + 4 * g);  // broadcast LDS reads
    const u32v4 kb = *reinterpret_cast<const u32v4 *>(lb + 4 * g);
    c += __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
    cA += __popc(v.x & ka.x) + __popc(v.y & ka.y) + __popc(v.z & ka.z) + __popc(v.w & ka.w);
    cB += __popc(v.x & kb.x) + __popc(v.y & kb.y) + __popc(v.z & kb.z) + __popc(v.w & kb.w);
    if (SUBSET_P) {
        const u32v4 kp = *reinterpret_cast<const u32v4 *>(lp + 4 * g);
        cP += __popc(v.x & kp.x) + __popc(v.y & kp.y) + __popc(v.z & kp.z) + __popc(v.w & kp.w);
    }
}

template <bool SUBSET_P, bool WEIGHTED>
__global__ __launch_bounds__(256, 4) void scan_tiles_anyn_kernel(const uint32_t *__restrict__ sb, const uint64_t *__restrict__ rare,
                                                                 const ScanTile *__restrict__ tiles,
                                                                 const uint32_t *__restrict__ masks, uint32_t wps, uint32_t G,
                                                                 uint32_t r, const PopSizes ps, const uint32_t *__restrict__ weights,
                                                                 TilePartial *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) uint32_t an_lds[];  // p | a | b, each padded to a multiple of 4 dwords
    const uint32_t wps4 = (wps + 3) & ~3u;
    uint32_t *lp = an_lds, *la = an_lds + wps4, *lb = an_lds + 2 * wps4;
    for (uint32_t k = threadIdx.x; k < wps4; k += 256) {
        const bool in = k < wps;
        lp[k] = in ? masks[k] : 0u; la[k] = in ? masks[wps + k] : 0u; lb[k] = in ? masks[2 * wps + k] : 0u;
    }
    __syncthreads();
    const ScanTile t = tiles[blockIdx.x];
    const auto [b0, b1, lane, wave] = tile_blocks_of(t);
    const uint32_t Gf = sb_full_granules(G, r);
    LaneAcc acc;
    for (uint64_t b = b0 + wave; b < b1; b += 4) {
        const uint32_t *blk = sb + b * 64ull * wps;
        uint32_t c = 0, cP = 0, cA = 0, cB = 0;
        // the last granule's r = 1..3 dwords per site go out first, together with the first batch
        uint32_t tail[3] = {0u, 0u, 0u};
        sb_load_tail(blk, G, r, lane, tail);
        // full batches of AN_U granules (all loads out first, consumed with staggered waits) ...
        uint32_t g = 0;
        for (; g + AN_U <= Gf; g += AN_U) {
            u32v4 v[AN_U];
            sb_load_granules(blk, g, AN_U, lane, v);
#pragma unroll
            for (int u = 0; u < AN_U; ++u) anyn_granule<SUBSET_P>(v[u], lp, la, lb, g + u, c, cP, cA, cB);
        }
        // ... and ONE short batch for what is left (wave-uniform predicates): its loads still go out together; a
        // one-at-a-time remainder loop paid the full HBM latency per granule
        if (g < Gf) {
            const uint32_t nb = Gf - g;
            u32v4 v[AN_U - 1];
            sb_load_granules(blk, g, nb, lane, v);
#pragma unroll
            for (int u = 0; u < AN_U - 1; ++u)
                if ((uint32_t)u < nb) anyn_granule<SUBSET_P>(v[u], lp, la, lb, g + u, c, cP, cA, cB);
        }
        sb_use_tail(G, r, tail, [&](uint32_t k, uint32_t v) {
            c += __popc(v); cA += __popc(v & la[k]); cB += __popc(v & lb[k]);
            if (SUBSET_P) cP += __popc(v & lp[k]);
        });
        const uint64_t s = b * 64 + lane;
        if (s >= t.site_begin && s < t.site_end)  // only the first / last block of a tile is partial
            counts_accumulate<SUBSET_P>(c, cP, cA, cB, ps, acc, WEIGHTED ? weights[s] : 1);
    }
    if constexpr (!WEIGHTED) {  // weighted matrices never stream the split index
        if (t.rare_end > t.rare_begin) rare_range<SUBSET_P>(rare, t.rare_begin, t.rare_end, lp, la, lb, ps, acc);
    }
    tile_reduce_store(acc, out);
}

// TPW threads per window sum its tile partials (integers: any order gives the same totals), then one thread
// runs the fp64 epilogue.  Same operation order as oracle_window_sitecount (oracle/impop_oracle.c) which restates
// pica2.py:154,164, h-fst.py:203-240 and tj_d.py:53-65 on the exact pair sums.  TPW = 1 for the usual many-
// windows-of-a-few-tiles shape, 64 (a wave per window) / 256 (a workgroup per window) when windows span many
// tiles — BASELINE config 5's single 10^7-site window is ~19 500 tiles, a 0.9 MB read that one thread would
// walk serially behind the streaming kernel.
struct WinTotals {
    uint32_t s_all, s_p, s_a, s_b;
    uint64_t sum_p, sum_a, sum_b, sum_ab;
};

// Hudson Fst of populations A, B from a window's exact pair sums (h-fst.py:203-240): W = window length or weight.  The order
// of the fp64 operations is the parity contract with the reference.
__device__ __forceinline__ impop_pair_stats hudson_fst(uint64_t sum_a, uint64_t sum_b, uint64_t sum_ab, uint32_t n_a, uint32_t n_b,
                                                       double W, double seq_len) {
    const double nA = (double)n_a, nB = (double)n_b;
    const double pairsA = nA * (nA - 1.0) / 2.0, pairsB = nB * (nB - 1.0) / 2.0;
    impop_pair_stats r;
    r.pi_a = (n_a >= 2 && W > 0) ? (double)sum_a / (pairsA * W) : 0.0;
    r.pi_b = (n_b >= 2 && W > 0) ? (double)sum_b / (pairsB * W) : 0.0;
    r.dxy = (n_a && n_b && W > 0) ? (double)sum_ab / (nA * nB * W) : 0.0;
    r.pi_xy = 0.5 * (r.pi_a + r.pi_b);
    r.fst = (r.dxy > 0) ? (r.dxy - r.pi_xy) / r.dxy : 0.0;
    r.da = r.dxy - r.pi_xy;
    if (seq_len > 0) {
        r.pi_a /= seq_len; r.pi_b /= seq_len; r.da = (r.dxy - r.pi_xy) / seq_len; r.pi_xy /= seq_len; r.dxy /= seq_len;
    }
    return r;
}

__device__ inline void window_epilogue(const WinDesc &w, const WinTotals &T, const PopSizes &ps, const double *__restrict__ taj,
                                       int d_pi_mode, int s_scope, impop_window_stats *__restrict__ dst) {
    const uint64_t n_sites = w.n_sites;  // window length, or the sum of its columns' weights (window_weights)
    impop_window_stats r;
    r.n_sites = (uint32_t)n_sites;       // <= 2^32 - 1 by the plan-time checks
    r.s_all = T.s_all; r.s_p = T.s_p; r.s_a = T.s_a; r.s_b = T.s_b; r.flags = 0;
    r.sum_p = T.sum_p; r.sum_a = T.sum_a; r.sum_b = T.sum_b; r.sum_ab = T.sum_ab;
    const double nan = __builtin_nan("");
    const double W = (double)n_sites;
    const double seq_len = (double)w.seq_len;
    const double nP = (double)ps.nP;
    const double pairsP = nP * (double)(ps.nP - 1) / 2.0;
    const double pi = (ps.nP >= 2 && W > 0) ? (double)T.sum_p / (pairsP * W) : 0.0;
    const double pi_site = (seq_len != 0.0) ? pi / seq_len : nan;
    const impop_pair_stats h = hudson_fst(T.sum_a, T.sum_b, T.sum_ab, ps.nA, ps.nB, W, seq_len);
    r.pi = pi; r.pi_site = pi_site; r.pi_a = h.pi_a; r.pi_b = h.pi_b; r.pi_xy = h.pi_xy; r.dxy = h.dxy; r.da = h.da; r.fst = h.fst;
    const double S = (double)(s_scope == 0 ? T.s_all : T.s_p);
    const double pin = d_pi_mode == 0 ? py_round(pi_site, 8) : d_pi_mode == 1 ? pi_site : pi * W;
    double D = nan;
    if (ps.nP >= 2 && pin == pin) {
        TajConsts c;
        c.a1 = taj[0]; c.a2 = taj[1]; c.b1 = taj[2]; c.b2 = taj[3]; c.c1 = taj[4]; c.c2 = taj[5]; c.e1 = taj[6]; c.e2 = taj[7];
        D = tajima_d_from(c, S, pin, nullptr, nullptr);
    }
    r.tajima_d = D;
    *dst = r;
}

template <int TPW>
__global__ __launch_bounds__(TPW == 1 ? 128 : 256) void scan_finalize_kernel(const TilePartial *__restrict__ parts,
                                                                             const WinDesc *__restrict__ wins, uint64_t n_windows,
                                                                             PopSizes ps, const double *__restrict__ taj,
                                                                             int d_pi_mode, int s_scope,
                                                                             impop_window_stats *__restrict__ out) {
    constexpr int BLOCK = TPW == 1 ? 128 : 256;
    const uint64_t i = ((uint64_t)blockIdx.x * BLOCK + threadIdx.x) / TPW;  // uniform per wave for TPW >= 64
    const uint32_t sub = threadIdx.x % TPW;
    if (TPW < 256 && i >= n_windows) return;
    const WinDesc w = wins[i];
    WinTotals T = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint64_t t = w.t0 + sub; t < w.t1; t += TPW) {
        const TilePartial p = parts[t];
        T.s_all += p.s_all; T.s_p += p.s_p; T.s_a += p.s_a; T.s_b += p.s_b;
        T.sum_p += p.sum_p; T.sum_a += p.sum_a; T.sum_b += p.sum_b; T.sum_ab += p.sum_ab;
    }
    if (TPW >= 64) {
        T.s_all = wave_sum_u32(T.s_all); T.s_p = wave_sum_u32(T.s_p); T.s_a = wave_sum_u32(T.s_a); T.s_b = wave_sum_u32(T.s_b);
        T.sum_p = wave_sum_u64(T.sum_p); T.sum_a = wave_sum_u64(T.sum_a); T.sum_b = wave_sum_u64(T.sum_b);
        T.sum_ab = wave_sum_u64(T.sum_ab);
    }
    if (TPW == 256) {
        __shared__ WinTotals red[4];
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = T;
        __syncthreads();
        if (threadIdx.x == 0)
            for (int k = 1; k < 4; ++k) {
                T.s_all += red[k].s_all; T.s_p += red[k].s_p; T.s_a += red[k].s_a; T.s_b += red[k].s_b;
                T.sum_p += red[k].sum_p; T.sum_a += red[k].sum_a; T.sum_b += red[k].sum_b; T.sum_ab += red[k].sum_ab;
            }
    }
    if (sub == 0) window_epilogue(w, T, ps, taj, d_pi_mode, s_scope, out + i);
}

// c = sum_k popc(dword_k & mask_k) of site `lane` of a block; masks wave-uniform
__device__ __forceinline__ uint32_t masked_site_count(const uint32_t *__restrict__ blk, const uint32_t *__restrict__ mask, uint32_t G,
                                                      uint32_t r, uint32_t lane) {
    uint32_t c = 0;
    sb_for_each_dword<true>(blk, G, r, lane, [&](uint32_t k, uint32_t w) { c += __popc(w & mask[k]); });
    return c;
}

__global__ __launch_bounds__(256) void site_counts_kernel(const uint32_t *__restrict__ sb, const uint32_t *__restrict__ mask,
                                                          uint32_t wps, uint32_t G, uint32_t r, uint64_t site_begin,
                                                          uint64_t site_end, uint32_t *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t b = (site_begin >> 6) + (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint64_t s = b * 64 + lane;
    if (s < site_begin || s >= site_end) return;
    out[s - site_begin] = masked_site_count(sb + b * 64ull * wps, mask, G, r, lane);
}

// ---- K disjoint populations in one pass: all-pairs Hudson Fst (run_h_fst_panels.sh:60-71) -------
// Per tile: sum_k c_k (n_k - c_k) for every population and sum_s [c_k (n_l - c_l) + c_l (n_k - c_k)] for
// every pair k < l.  Masks come from memory (wave-uniform scalar loads); K is a template parameter so
// that the per-lane accumulators are registers.  out: tile-major, K + K(K-1)/2 uint64 per tile.
// Round 2: masks of all K populations in LDS (K x wps dwords, broadcast ds_read_b128), granules loaded four at a time
// (the first version had ONE load in flight per wave), and for unweighted matrices of <= 512 haplotypes (SMALL) the
// per-site work is K + K + K(K-1)/2 32-bit multiply-adds — sum c_k, sum c_k^2, sum c_k c_l — from which the tile's
//   sum_s c_k (n_k - c_k) = n_k sum c_k - sum c_k^2,   sum_s [c_k (n_l - c_l) + c_l (n_k - c_k)] = n_l sum c_k + n_k sum c_l - 2 sum c_k c_l
// follow once per lane and tile (every partial sum stays below 2^32: <= 1024 sites per lane and tile, products < 2^18);
// the first version did three to four 64-bit multiplies per pair and site, which made K = 8 VALU-bound.
template <int K, bool SMALL>
__global__ __launch_bounds__(256) void scan_multi_kernel(const uint32_t *__restrict__ sb, const uint64_t *__restrict__ rare,
                                                         const ScanTile *__restrict__ tiles,
                                                         const uint32_t *__restrict__ masks /* K x wps */,
                                                         const uint32_t *__restrict__ pop_n /* K */, uint32_t wps,
                                                         uint32_t G, uint32_t r, const uint32_t *__restrict__ weights /* nullable */,
                                                         uint64_t *__restrict__ out) {
    constexpr int NP = K * (K - 1) / 2;
    extern __shared__ __attribute__((aligned(16))) uint32_t mk_lds[];  // K x wps4
    pop_masks_to_lds<K>(mk_lds, masks, wps);
    __syncthreads();
    const ScanTile t = tiles[blockIdx.x];
    const TileBlocks tb = tile_blocks_of(t);
    uint32_t nk[K];
#pragma unroll
    for (int k = 0; k < K; ++k) nk[k] = pop_n[k];
    uint64_t acc[K + NP];
    uint32_t s1[K], q2[K], px[NP > 0 ? NP : 1];
#pragma unroll
    for (int i = 0; i < K + NP; ++i) acc[i] = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) { s1[k] = 0; q2[k] = 0; }
#pragma unroll
    for (int i = 0; i < NP; ++i) px[i] = 0;
    // wt: the site's weight (unweighted: 1)
    auto tally_counts = [&](const uint32_t (&c)[K], uint64_t wt) {
        if (SMALL) {
            int pi = 0;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                s1[k] += c[k];
                q2[k] += __umul24(c[k], c[k]);
#pragma unroll
                for (int l = k + 1; l < K; ++l) px[pi++] += __umul24(c[k], c[l]);
            }
        } else {
            int pi = K;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                acc[k] += wt * (c[k] * (nk[k] - c[k]));
#pragma unroll
                for (int l = k + 1; l < K; ++l) acc[pi++] += wt * (c[k] * (nk[l] - c[l]) + c[l] * (nk[k] - c[k]));
            }
        }
    };
    pop_stream_tile<K, true>(
        sb, rare, t, tb, mk_lds, pop_n, wps, G, r,
        [&](const uint32_t (&c)[K], uint64_t s) { tally_counts(c, !SMALL && weights ? weights[s] : 1); },  // wave-uniform choice
        [&](const uint32_t (&c)[K]) { tally_counts(c, 1); });
    if (SMALL) {
        int pi = K;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            acc[k] = (uint64_t)nk[k] * s1[k] - q2[k];
#pragma unroll
            for (int l = k + 1; l < K; ++l) { acc[pi] = (uint64_t)nk[l] * s1[k] + (uint64_t)nk[k] * s1[l] - 2ull * px[pi - K]; ++pi; }
        }
    }
    tile_partials_store<K + NP>(tb, out, [&](int i) { return wave_sum_u64(acc[i]); });
}

// one thread per (window, pair): h-fst.py:203-240 on the exact pair sums
__global__ void scan_multi_finalize_kernel(const uint64_t *__restrict__ parts, const WinDesc *__restrict__ wins,
                                           uint64_t n_windows, uint32_t K, const uint32_t *__restrict__ pop_n,
                                           impop_pair_stats *__restrict__ out) {
    const uint32_t NP = K * (K - 1) / 2, stride = K + NP;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_windows * NP) return;
    const uint64_t win = i / NP;
    uint32_t p = (uint32_t)(i % NP), k = 0;
    while (p >= K - 1 - k) { p -= K - 1 - k; ++k; }
    const uint32_t l = k + 1 + p;
    const WinDesc w = wins[win];
    uint64_t sk = 0, sl = 0, skl = 0;
    for (uint64_t t = w.t0; t < w.t1; ++t) {
        sk += parts[t * stride + k];
        sl += parts[t * stride + l];
        skl += parts[t * stride + K + (uint32_t)(i % NP)];
    }
    out[i] = hudson_fst(sk, sl, skl, pop_n[k], pop_n[l], (double)w.n_sites, (double)w.seq_len);
}

// ---- allele-frequency spectrum (scripts/wip/op-afs.py): per window, how many sites carry c copies ----
// grid (chunks of 4096 sites, windows); LDS histogram per workgroup, integer atomics to the output.
__global__ __launch_bounds__(256) void afs_kernel(const uint32_t *__restrict__ sb, const uint32_t *__restrict__ mask,
                                                  uint32_t wps, uint32_t G, uint32_t r, const impop_window *__restrict__ wins,
                                                  uint32_t bins, uint64_t chunk_sites, uint32_t *__restrict__ out) {
    extern __shared__ uint32_t hist[];
    const impop_window w = wins[blockIdx.y];
    const uint64_t c0 = w.site_begin + (uint64_t)blockIdx.x * chunk_sites;
    if (c0 >= w.site_end) return;  // uniform per workgroup
    const uint64_t c1 = c0 + chunk_sites < w.site_end ? c0 + chunk_sites : w.site_end;
    for (uint32_t i = threadIdx.x; i < bins; i += 256) hist[i] = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // Most sites of a real matrix are carried by nobody or by everybody: those two bins are counted per WAVE (a ballot
    // and a popcount, one LDS add by one lane) — 64 lanes adding to the same LDS word one after the other was what this
    // kernel spent its time on; the bins in between keep their per-lane atomics (few lanes, spread over many words).
    uint32_t n_zero = 0, n_full = 0;
    for (uint64_t b = (c0 >> 6) + wave; b <= ((c1 - 1) >> 6); b += 4) {
        const uint64_t s = b * 64 + lane;
        const bool in = s >= c0 && s < c1;
        const uint32_t c = masked_site_count(sb + b * 64ull * wps, mask, G, r, lane);
        const bool zero = in && c == 0, full = in && !zero && c == bins - 1;  // an empty mask has ONE bin: count it once
        n_zero += (uint32_t)__popcll(__ballot(zero));
        n_full += (uint32_t)__popcll(__ballot(full));
        if (in && !zero && !full) atomicAdd(&hist[c], 1u);
    }
    if (lane == 0) {
        if (n_zero) atomicAdd(&hist[0], n_zero);
        if (n_full) atomicAdd(&hist[bins - 1], n_full);
    }
    __syncthreads();
    uint32_t *o = out + (uint64_t)blockIdx.y * bins;
    if (gridDim.x == 1) {  // the window's only workgroup: its histogram IS the result
        for (uint32_t i = threadIdx.x; i < bins; i += 256) o[i] = hist[i];
    } else {
        for (uint32_t i = threadIdx.x; i < bins; i += 256)
            if (hist[i]) atomicAdd(&o[i], hist[i]);
    }
}

// mask bitset (uint64 words, n bits) -> wps dwords clipped to n; NULL -> `fill`
static void mask_to_dwords(const uint64_t *mask, uint32_t n, uint32_t wps, bool fill_all, std::vector<uint32_t> &out) {
    out.assign(wps, 0u);
    for (uint32_t k = 0; k < wps; ++k) {
        uint32_t v;
        if (mask) v = (uint32_t)(mask[k >> 1] >> (32 * (k & 1)));
        else v = fill_all ? 0xFFFFFFFFu : 0u;
        const uint32_t lo = 32 * k;
        if (lo + 32 > n) v &= (n > lo) ? (uint32_t)((1ull << (n - lo)) - 1ull) : 0u;
        out[k] = v;
    }
}
static uint32_t popcount_vec(const std::vector<uint32_t> &v) {
    uint32_t c = 0;
    for (uint32_t x : v) c += (uint32_t)__builtin_popcount(x);
    return c;
}

}  // namespace impop

using namespace impop;

struct impop_scan_plan {
    impop_ctx *ctx = nullptr;
    const impop_matrix *m = nullptr;
    const uint32_t *sb = nullptr;  // the layout launches stream: m->d_vsb (route "indexed", tiles in kept-site coordinates) or m->d_sb
    const uint64_t *rare = nullptr;  // split index: m->d_vrare (tiles' rare ranges), packed route: m->d_vmulti, else null
    const uint16_t *single = nullptr;  // packed route: m->d_vsingle and every tile's range of it, else null
    SingleRange *d_singles = nullptr;
    const uint32_t *uniq = nullptr;  // unique-row route: m->d_vuniq, m->d_vuniq_wt and every tile's range of them, else null
    const uint8_t *uniq_wt = nullptr;
    UniqRange *d_uniqs = nullptr;
    bool wave_tiles = false;  // unique-row route: launches run scan_tiles_kernel_wave, one wave per tile (tile_cut.h, wave_tile_choice)
    // tile digest (tile_digest.h): one allocation of rows | weights | histograms and every tile's descriptor; launches then run
    // scan_tiles_kernel_digest.  d_digest null: none, digest_why says why
    void *d_digest = nullptr;
    DigestDesc *d_descs = nullptr;
    uint64_t digest_weight_off = 0, digest_hist_off = 0;
    uint64_t digest_rows = 0, digest_hist_tiles = 0, digest_bytes = 0;
    std::string digest_why = "not a scan plan of the one-wave body";
    uint64_t n_windows = 0, n_tiles = 0, bytes_streamed = 0;
    PopSizes ps{};
    bool subset_p = false;
    std::vector<uint32_t> masks;  // p | a | b, wps dwords each
    int d_pi_mode = 0, s_scope = 0;
    int finalize_tpw = 1;  // threads per window of scan_finalize_kernel: 1, 64 or 256 by the longest tile range
    ScanTile *d_tiles = nullptr;
    WinDesc *d_wins = nullptr;
    TilePartial *d_parts = nullptr;
    uint32_t *d_masks = nullptr;
    // Tajima's constants for the plan's nP (8 doubles, tajima_consts_kernel), the plan's own: written at creation and by a
    // set_masks that changes nP, read by every finalize launch.  A launch touches no state of the context, so one captured
    // at any moment replays right whatever other plans and calls of the context did in between
    double *d_taj = nullptr;
    int64_t taj_n = -1;  // the n d_taj holds, or was last queued to hold
    impop_window_stats *d_out = nullptr;
    bool timing = false;
    EventPairs timer;  // one pair per timed launch of the streaming kernel
};

// W of every window in ORIGINAL coordinates: its length, or the sum of its columns' weights (tiles of compacted matrices and
// of indexed plans are in kept-site coordinates, so cut_tiles' lengths are not the windows')
static int window_weights(const impop_matrix *m, const impop_window *windows, uint64_t n_windows, ScanRoute &rt) {
    for (uint64_t i = 0; i < n_windows; ++i) {
        uint64_t &W = rt.wins[i].n_sites;
        if (!m->wt_prefix.empty()) {
            W = m->wt_prefix[windows[i].site_end] - m->wt_prefix[windows[i].site_begin];
            // impop_window_stats.n_sites is 32 bits wide: refuse rather than truncate (unweighted windows are
            // checked against the same limit by their length)
            REQUIRE(W <= 0xFFFFFFFFull, "window %llu: the weights of its columns add up to %llu >= 2^32; split the window",
                    (unsigned long long)i, (unsigned long long)W);
        } else if (m->compact || rt.indexed) {
            W = windows[i].site_end - windows[i].site_begin;
        }
    }
    return IMPOP_OK;
}

// The default tile (tile_cut.h, default_tile_rule).  The blocks the windows cover are counted in the coordinates of the layout
// streamed (a compacted matrix: in the original ones) and capped at that layout's length, which overlapping windows exceed; the
// rare sites of a split index, whichever stream holds them, count as the blocks of rows their 8-byte entries would fill.
static uint32_t default_tile_blocks(const impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, const ScanRoute &rt) {
    uint64_t blocks = 0, entries = 0;
    for (size_t i = 0; i < rt.lw.size(); ++i) {
        const LayoutWindow &w = rt.lw[i];
        blocks += ((rt.indexed ? w.hi.c - w.lo.c : windows[i].site_end - windows[i].site_begin) + 63) / 64;
        entries += (w.hi.r - w.lo.r) + (w.hi.g - w.lo.g);
    }
    if (m->compact && blocks > m->g.n_block) blocks = m->g.n_block;
    if (rt.indexed && blocks > m->vg.n_block) blocks = m->vg.n_block;
    if (entries > m->n_vrare) entries = m->n_vrare;
    return default_tile_rule(m->g.wps, blocks + entries * 8 / (64ull * m->g.wps * 4ull), ctx->n_cu);
}

// subset masks of a plan; the overlap of A and B is removed from both (h-fst.py:181-185)
static void plan_set_masks(impop_scan_plan *p, const uint64_t *mask_p, const uint64_t *mask_a, const uint64_t *mask_b) {
    const uint32_t n = p->m->g.n_hap, wps = p->m->g.wps;
    std::vector<uint32_t> mp, ma, mb;
    mask_to_dwords(mask_p, n, wps, true, mp);
    mask_to_dwords(mask_a, n, wps, false, ma);
    mask_to_dwords(mask_b, n, wps, false, mb);
    for (uint32_t k = 0; k < wps; ++k) {
        const uint32_t ov = ma[k] & mb[k];
        ma[k] &= ~ov; mb[k] &= ~ov;
    }
    p->ps.n = n; p->ps.nP = popcount_vec(mp); p->ps.nA = popcount_vec(ma); p->ps.nB = popcount_vec(mb);
    p->subset_p = p->ps.nP != n;
    p->masks.clear();
    p->masks.reserve(3 * wps);
    p->masks.insert(p->masks.end(), mp.begin(), mp.end());
    p->masks.insert(p->masks.end(), ma.begin(), ma.end());
    p->masks.insert(p->masks.end(), mb.begin(), mb.end());
}

// queues the constants of the plan's nP into its own slot on the context's stream, where the slot holds another n's
static int plan_fill_tajima(impop_scan_plan *p) {
    const int64_t n = p->ps.nP >= 2 ? (int64_t)p->ps.nP : 2;
    if (p->taj_n == n) return IMPOP_OK;
    const int rc = fill_tajima_consts(p->ctx, n, p->d_taj);
    if (rc) return rc;
    p->taj_n = n;
    return IMPOP_OK;
}

// IMPOP_TRACE=1: one line per plan (and per impop_scan_multi) with the route it streams; tests read it.  kept_sites = every
// variable site of an indexed route; rare_sites / rare_bytes = the split index's rare entries (all of the matrix / the plan's);
// split = on, or off:<the reason there is none, blanks as _>; single_sites = the singleton stream of a packed route (all of the
// matrix), rare_streamed = the bytes of rare sites the plan really reads (rare_bytes keeps counting 8 per rare site);
// unique_rows = the representatives of the distinct-row stream of a unique-row route (all of the matrix), rows_streamed = the
// bytes of rows the plan really reads (bytes_streamed = rows_streamed + rare_streamed); wave_tiles = 1 where the fixed-WPS kernel
// will run one wave per tile; digest = 1 where it will run from the plan's tile digest, and the three byte counts are then what
// such a launch reads (the last key; the free-text why= stays behind it, where the parsers that cut the line there expect it)
void impop::trace_route(const impop_matrix *m, const ScanRoute &rt, uint64_t n_windows) {
    if (!trace_on()) return;
    const char *why = rt.indexed || m->compact ? "" : !m->wt_prefix.empty() && m->d_vsb ? "site weights" : m->vskip.c_str();
    uint64_t rare_bytes = 0, rare_streamed = 0;
    for (const ScanTile &t : rt.tiles) rare_bytes += (t.rare_end - t.rare_begin) * 8ull;
    rare_streamed = rare_bytes;
    for (const SingleRange &r : rt.singles) { rare_bytes += (r.end - r.begin) * 8ull; rare_streamed += single_bytes_streamed(r); }
    if (rt.digest) rare_streamed = rt.digest_rare_streamed;
    const uint64_t rows_streamed = rt.bytes_streamed - rare_streamed;
    std::string off = "off:" + (!m->wt_prefix.empty() && m->d_vrare ? std::string("site weights") : m->rskip);
    for (char &ch : off) ch = ch == ' ' ? '_' : ch;
    fprintf(stderr, "[impop_scan] route=%s kept_sites=%llu tiles=%llu bytes_streamed=%llu windows=%llu rare_sites=%llu rare_bytes=%llu split=%s single_sites=%llu rare_streamed=%llu unique_rows=%llu rows_streamed=%llu wave_tiles=%d digest=%d%s%s\n",
            rt.indexed ? "indexed" : m->compact ? "compact" : "dense", (unsigned long long)(rt.indexed ? m->n_vkept : m->g.n_site),
            (unsigned long long)rt.tiles.size(), (unsigned long long)rt.bytes_streamed, (unsigned long long)n_windows,
            (unsigned long long)(rt.split ? m->n_vrare : 0), (unsigned long long)rare_bytes, rt.split ? "on" : off.c_str(), (unsigned long long)(rt.packed ? m->n_vsingle : 0),
            (unsigned long long)rare_streamed, (unsigned long long)(rt.uniq ? m->n_vuniq : 0), (unsigned long long)rows_streamed,
            rt.wave_tiles ? 1 : 0, rt.digest ? 1 : 0, *why ? " why=" : "", why);
    fflush(stderr);  // in order with the caller's own stderr lines even where stderr is buffered
}

// unique-row route: every tile's range of the distinct-row stream, from the tiles and the stream's per-block prefix where that
// lives, on the device (one thread per tile), and back once: bytes_streamed stays the bytes a launch reads
__global__ void uniq_ranges_kernel(const ScanTile *__restrict__ tiles, uint64_t n_tiles, const uint64_t *__restrict__ ubase,
                                   uint32_t wps, UniqRange *__restrict__ out) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n_tiles) out[k] = uniq_range_of(tiles[k].site_begin, tiles[k].site_end, ubase, wps);
}
static int tile_uniq_ranges(impop_ctx *ctx, const impop_matrix *m, ScanRoute &rt) {
    const size_t nt = rt.tiles.size();
    rt.uniqs.resize(nt);
    if (!nt) return IMPOP_OK;
    REQUIRE((nt + 255) / 256 < 0x7FFFFFFFull, "impop_scan: too many tiles for one launch");
    Carve L;
    const size_t o_in = L.take<ScanTile>(nt), o_out = L.take<UniqRange>(nt);
    void *d = nullptr;
    const int rc = ctx_aux(ctx, 0, L.total(), &d);  // as map_windows_index: idle outside the all-pairs path
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(L.at<ScanTile>(d, o_in), rt.tiles.data(), nt * sizeof(ScanTile), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(uniq_ranges_kernel, dim3((uint32_t)((nt + 255) / 256)), dim3(256), 0, ctx->stream,
                       (const ScanTile *)L.at<ScanTile>(d, o_in), (uint64_t)nt, m->uidx.base, m->g.wps, L.at<UniqRange>(d, o_out));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(rt.uniqs.data(), L.at<UniqRange>(d, o_out), nt * sizeof(UniqRange), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return IMPOP_OK;
}

// ---- the tile digest of a plan (tile_digest.h), built on the device where the plan is made ----
// One workgroup per tile.  The tile's candidate rows — head rows, representatives of the distinct-row stream with their weights,
// tail rows; every row where the tile has no range of the stream — are brought to canonical form in LDS (a row whose haplotype 0
// carries 1 is complemented within the n_hap real haplotypes: a row and its complement then are the same words, padding bits
// zero), and candidate i is a representative unless an earlier candidate has its hash and its words: first occurrence, so the
// order is the rows' own and the same at every build.  The weights of a class add up in LDS (integers: any order).
// Count pass (n_reps not null): the tile's number of representatives.  Write pass (descs not null): its rows and weights at the
// place digest_layout gave it, rank = the representatives before it, and its singleton histogram where it has one.
// A tile above DIGEST_ROWS_MAX candidates is refused by the host before any launch; the kernel leaves it alone all the same.
__global__ __launch_bounds__(256) void digest_build_kernel(const uint32_t *__restrict__ sb, const uint32_t *__restrict__ uniq,
                                                           const uint8_t *__restrict__ uniq_wt, const ScanTile *__restrict__ tiles,
                                                           const UniqRange *__restrict__ uniqs, uint32_t n_hap, uint32_t wps,
                                                           uint32_t G, uint32_t r, uint32_t *__restrict__ n_reps,
                                                           const DigestDesc *__restrict__ descs, uint32_t *__restrict__ rows,
                                                           uint16_t *__restrict__ wts, const uint16_t *__restrict__ single,
                                                           const SingleRange *__restrict__ singles, uint16_t *__restrict__ hists) {
    constexpr uint32_t MAXC = (uint32_t)DIGEST_ROWS_MAX;
    __shared__ uint32_t cand[MAXC * 16];  // wps <= 16 dwords per candidate
    __shared__ uint32_t hash[MAXC], wsum[MAXC], hist[MAXC];
    __shared__ uint16_t cwt[MAXC], first[MAXC];
    __shared__ uint32_t n_rep;
    const uint32_t k = blockIdx.x, tid = threadIdx.x;
    const ScanTile t = tiles[k];
    const UniqRange ur = uniqs[k];
    const bool folded = ur.end > ur.begin, any = t.site_end > t.site_begin;
    const MidBlocks mid = mid_blocks(t.site_begin, t.site_end);
    const uint64_t head_end = folded ? mid.g0 << 6 : t.site_end, tail_begin = folded ? mid.g1 << 6 : t.site_end;
    const uint64_t nh64 = any ? head_end - t.site_begin : 0, nu64 = folded ? ur.end - ur.begin : 0, nt64 = any ? t.site_end - tail_begin : 0;
    if (nh64 + nu64 + nt64 > MAXC || wps > 16) {  // uniform
        if (n_reps && tid == 0) n_reps[k] = 0xFFFFFFFFu;
        return;
    }
    const uint32_t nh = (uint32_t)nh64, nu = (uint32_t)nu64, nc = nh + nu + (uint32_t)nt64;
    const uint32_t last_mask = (n_hap & 31u) ? (1u << (n_hap & 31u)) - 1u : 0xFFFFFFFFu;
    if (tid == 0) n_rep = 0;
    for (uint32_t i = tid; i < nc; i += 256) {
        const bool rep = i >= nh && i < nh + nu;
        const uint64_t s = i < nh ? t.site_begin + i : rep ? ur.begin + (i - nh) : tail_begin + (i - nh - nu);
        const uint32_t *src = rep ? uniq : sb;
        const uint64_t blk = s >> 6;
        const uint32_t l = (uint32_t)(s & 63);
        const bool flip = (src[sb_index(wps, G, r, blk, l, 0)] & 1u) != 0;
        uint32_t h = 2166136261u;
        for (uint32_t q = 0; q < wps; ++q) {
            uint32_t v = src[sb_index(wps, G, r, blk, l, q)];
            if (flip) v ^= q + 1 == wps ? last_mask : 0xFFFFFFFFu;
            cand[i * wps + q] = v;
            h = (h ^ v) * 16777619u;
        }
        hash[i] = h;
        wsum[i] = 0;
        cwt[i] = rep ? (uint16_t)uniq_wt[s] : (uint16_t)1;
    }
    __syncthreads();
    for (uint32_t i = tid; i < nc; i += 256) {
        uint32_t f = i;
        for (uint32_t j = 0; j < i; ++j) {
            if (hash[j] != hash[i]) continue;
            bool same = true;
            for (uint32_t q = 0; q < wps; ++q) same = same && cand[j * wps + q] == cand[i * wps + q];
            if (same) { f = j; break; }
        }
        first[i] = (uint16_t)f;
        atomicAdd(&wsum[f], (uint32_t)cwt[i]);
        if (f == i) atomicAdd(&n_rep, 1u);
    }
    __syncthreads();
    if (n_reps && tid == 0) n_reps[k] = n_rep;
    if (!descs) return;
    const DigestDesc d = descs[k];
    const uint32_t padded = (uint32_t)digest_rows_padded(d.n_rows);
    uint32_t *base = rows + d.row_off * wps;
    for (uint32_t i = tid; i < nc; i += 256) {
        if (first[i] != i) continue;
        uint32_t rank = 0;
        for (uint32_t j = 0; j < i; ++j) rank += first[j] == j;
        if (rank >= d.n_rows) continue;  // never: the count pass saw the same rows
        for (uint32_t q = 0; q < wps; ++q) {
            const uint32_t g = q >> 2;
            const uint64_t at = g + 1 < G ? ((uint64_t)g * padded + rank) * 4 + (q & 3u) : (uint64_t)(G - 1) * padded * 4 + (uint64_t)rank * r + (q - 4 * (G - 1));
            base[at] = cand[i * wps + q];
        }
        wts[d.row_off + rank] = (uint16_t)wsum[i];
    }
    if (d.hist == 0) return;  // uniform
    const uint32_t nh16 = 32u * wps;
    const SingleRange sr = singles[k];
    for (uint32_t h = tid; h < nh16; h += 256) hist[h] = 0;
    __syncthreads();
    for (uint64_t s = sr.begin + tid; s < sr.end; s += 256) {
        const uint32_t h = single[s] & 0x7FFFu;  // bit 15: which allele the carrier holds, nothing to a singleton's sums
        if (h < nh16) atomicAdd(&hist[h], 1u);
    }
    __syncthreads();
    uint16_t *dst = hists + (uint64_t)(d.hist - 1) * nh16;
    for (uint32_t h = tid; h < nh16; h += 256) dst[h] = (uint16_t)hist[h];
}

// Decides whether plan p, whose tables are queued for upload on the context's stream, takes a digest, and builds it: the caps
// and the rule of tile_digest.h, IMPOP_SCAN_DIGEST=0|1 overriding the rule.  The count pass and one small download give the host
// every tile's place; one allocation; the write pass.  On return rt counts what a launch of the plan reads.  reusable: the
// plan's maker may launch it again (impop_scan_plan_create), else a one-shot call made it, which the rule leaves without.
static int plan_build_digest(impop_scan_plan *p, ScanRoute &rt, bool reusable) {
    const impop_matrix *m = p->m;
    impop_ctx *ctx = p->ctx;
    const size_t nt = rt.tiles.size();
    const uint32_t wps = m->g.wps;
    if (!rt.wave_tiles || !nt) return IMPOP_OK;
    const int force = env_is("IMPOP_SCAN_DIGEST", '0') ? 0 : env_is("IMPOP_SCAN_DIGEST", '1') ? 1 : -1;
    bool all_fit = true;
    for (size_t k = 0; k < nt && all_fit; ++k) all_fit = digest_tile_fits(rt.tiles[k], rt.uniqs[k], rt.packed ? rt.singles[k] : SingleRange{0, 0});
    if (!digest_wanted(force, reusable, true, all_fit)) {
        p->digest_why = force == 0 ? "IMPOP_SCAN_DIGEST=0" : !all_fit ? "a tile holds more than the digest's caps" : "a one-shot scan does not pay for the build";
        return IMPOP_OK;
    }
    uint32_t *d_reps = nullptr;
    std::vector<uint32_t> reps(nt);
    auto launch = [&](uint32_t *n_reps, const DigestDesc *descs) {
        hipLaunchKernelGGL(digest_build_kernel, dim3((uint32_t)nt), dim3(256), 0, ctx->stream, m->d_vsb, m->d_vuniq, m->d_vuniq_wt,
                           (const ScanTile *)p->d_tiles, (const UniqRange *)p->d_uniqs, m->g.n_hap, wps, m->g.G, m->g.r, n_reps, descs,
                           (uint32_t *)p->d_digest, (uint16_t *)((char *)p->d_digest + p->digest_weight_off), p->single,
                           (const SingleRange *)p->d_singles, (uint16_t *)((char *)p->d_digest + p->digest_hist_off));
        return hipGetLastError();
    };
    HIP_TRY(hipMalloc((void **)&d_reps, nt * sizeof(uint32_t)));
    hipError_t e = launch(d_reps, nullptr);
    if (e == hipSuccess) e = hipMemcpyAsync(reps.data(), d_reps, nt * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    hipFree(d_reps);
    HIP_TRY(e);
    for (size_t k = 0; k < nt; ++k)
        REQUIRE(reps[k] <= DIGEST_ROWS_MAX, "impop_scan: tile %zu: the digest's count pass refused it", k);
    DigestLayout L;
    digest_layout(rt.tiles, rt.singles, reps.data(), wps, L);
    if (!digest_choice(force, reusable, true, all_fit, L.bytes_streamed(), rt.bytes_streamed)) {
        p->digest_why = "a launch would read more bytes with the digest than without";
        return IMPOP_OK;
    }
    HIP_TRY(hipMalloc(&p->d_digest, std::max<size_t>(L.alloc_bytes(), 16)));
    HIP_TRY(hipMalloc((void **)&p->d_descs, nt * sizeof(DigestDesc)));
    p->digest_weight_off = L.weight_offset(); p->digest_hist_off = L.hist_offset();
    HIP_TRY(hipMemsetAsync(p->d_digest, 0, std::max<size_t>(L.alloc_bytes(), 16), ctx->stream));  // the padding rows: zero words, weight 0
    HIP_TRY(hipMemcpyAsync(p->d_descs, L.descs.data(), nt * sizeof(DigestDesc), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(launch(nullptr, p->d_descs));
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // L dies at return
    p->digest_rows = L.n_rows; p->digest_hist_tiles = L.n_hist_tiles; p->digest_bytes = L.digest_bytes();
    p->digest_why.clear();
    rt.digest = true;
    rt.digest_rare_streamed = L.rare_streamed();
    rt.bytes_streamed = L.bytes_streamed();
    return IMPOP_OK;
}

// every window lies in the matrix and is at most 2^32 - 1 sites long (impop_window_stats.n_sites is 32 bits wide)
int impop::check_windows(const char *fn, const impop_matrix *m, const impop_window *windows, uint64_t n_windows) {
    for (uint64_t i = 0; i < n_windows; ++i) {
        REQUIRE(windows[i].site_begin <= windows[i].site_end && windows[i].site_end <= matrix_span(m),
                "%s: window %llu: bad site range [%llu,%llu) for %llu sites", fn, (unsigned long long)i,
                (unsigned long long)windows[i].site_begin, (unsigned long long)windows[i].site_end,
                (unsigned long long)matrix_span(m));
        REQUIRE(windows[i].site_end - windows[i].site_begin <= 0xFFFFFFFFull, "%s: window %llu longer than 2^32 sites", fn,
                (unsigned long long)i);
    }
    return IMPOP_OK;
}

std::vector<LayoutWindow> impop::row_windows(const impop_matrix *m, const impop_window *windows, uint64_t n_windows) {
    std::vector<impop_window> mapped;
    map_windows(m, windows, n_windows, mapped);
    std::vector<LayoutWindow> lw(n_windows);
    for (uint64_t i = 0; i < n_windows; ++i) lw[i] = {{mapped[i].site_begin, 0, 0}, {mapped[i].site_end, 0, 0}, mapped[i].seq_len};
    return lw;
}

int impop::check_window_weights(const char *fn, const impop_matrix *m, const impop_window *windows, uint64_t n_windows) {
    for (uint64_t i = 0; i < n_windows; ++i)
        REQUIRE(window_W(m, windows[i].site_begin, windows[i].site_end) <= 0xFFFFFFFFull,
                "%s: window %llu: the weights of its columns add up to 2^32 or more; split the window", fn, (unsigned long long)i);
    return IMPOP_OK;
}

// windows (validated, matrix coordinates) -> the route of a scan of m and what a launch on it streams: the variable-site
// index when the matrix has one and no site weights (d_wt is indexed by matrix site), with the rare-entry stream of a split
// index; else the matrix itself (compacted: original coordinates -> kept-site index ranges).  tile_blocks 0: the default.
int impop::scan_route(const char *fn, impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows,
                      uint32_t tile_blocks, ScanRoute &rt, bool want_packed, bool trace) {
    rt.indexed = m->d_vsb != nullptr && m->wt_prefix.empty();
    rt.split = rt.indexed && m->d_vrare != nullptr;
    rt.packed = want_packed && rt.split && m->d_vsingle != nullptr;
    rt.sb = rt.indexed ? m->d_vsb : m->d_sb;
    rt.rare = rt.packed ? m->d_vmulti : rt.split ? m->d_vrare : nullptr;
    rt.single = rt.packed ? m->d_vsingle : nullptr;
    if (rt.indexed) {
        const int rc = map_windows_index(ctx, m, windows, n_windows, rt.split ? rt.packed ? SINGLE : COMMON : KEPT, rt.lw);
        if (rc) return rc;
    } else {
        rt.lw = row_windows(m, windows, n_windows);
    }
    rt.tile_blocks = tile_blocks ? tile_blocks : default_tile_blocks(ctx, m, windows, rt);
    cut_tiles(rt.lw, rt.tile_blocks, m->g.wps, rt.packed, rt);
    int rc = IMPOP_OK;
    // unique-row route: the same tiles; each one's range of the distinct-row stream, whichever stream holds its rare sites
    if (want_packed && rt.split && m->d_vuniq) {
        rt.uniq = m->d_vuniq;
        rt.uniq_wt = m->d_vuniq_wt;
        if ((rc = tile_uniq_ranges(ctx, m, rt))) return rc;
        rt.apply_uniq_ranges(m->g.wps);
        // ... and which body of the kernel reads them: by the plan's largest tile, IMPOP_SCAN_WAVE_TILES=0|1 overriding the rule
        uint64_t max_blocks = 0, max_rare = 0;
        for (size_t k = 0; k < rt.tiles.size(); ++k) {
            max_blocks = std::max(max_blocks, tile_blocks_read(rt.tiles[k], rt.uniqs[k]));
            max_rare = std::max(max_rare, tile_rare_words(rt.tiles[k], rt.packed ? rt.singles[k] : SingleRange{0, 0}));
        }
        const int force = env_is("IMPOP_SCAN_WAVE_TILES", '0') ? 0 : env_is("IMPOP_SCAN_WAVE_TILES", '1') ? 1 : -1;
        rt.wave_tiles = wave_tile_choice(force, rt.tiles.size(), max_blocks, max_rare, ctx->n_cu);
    }
    rc = window_weights(m, windows, n_windows, rt);
    if (rc) return rc;
    REQUIRE(rt.tiles.size() < 0x7FFFFFFFull, "%s: %llu tiles exceed one launch; raise tile_blocks", fn,
            (unsigned long long)rt.tiles.size());
    if (trace) trace_route(m, rt, n_windows);
    return IMPOP_OK;
}

uint32_t impop::env_tile_blocks(const char *name) {
    const char *e = getenv(name);
    if (!e || !*e) return 0;
    const long v = strtol(e, nullptr, 10);
    return v < 1 ? 1u : v > 4096 ? 4096u : (uint32_t)v;
}

void impop::pop_panel_pack(const impop_matrix *m, const uint64_t *masks, uint32_t K, PopPanel &p) {
    const uint32_t n = m->g.n_hap, wps = m->g.wps, mwords = (n + 63) / 64;
    p.mk.clear();
    p.nk.resize(K);
    std::vector<uint32_t> one;
    for (uint32_t k = 0; k < K; ++k) {
        mask_to_dwords(masks + (size_t)k * mwords, n, wps, false, one);
        p.mk.insert(p.mk.end(), one.begin(), one.end());
        p.nk[k] = popcount_vec(one);
    }
}

int impop::pop_panel_upload(impop_ctx *ctx, const ScanRoute &rt, const PopPanel &p, PopPanelDev &dev,
                            const std::function<void(Layout &)> &own) {
    const size_t nt = rt.tiles.size(), nw = rt.wins.size();
    Layout L;
    L.sub(dev.tiles, std::max<size_t>(nt, 1));
    L.sub(dev.wins, nw);
    L.sub(dev.masks, p.mk.size());
    L.sub(dev.n, p.nk.size());
    own(L);
    void *d = nullptr;
    const int rc = ctx_scratch(ctx, L.total(), &d);
    if (rc) return rc;
    L.bind(d);
    if (nt) HIP_TRY(hipMemcpyAsync(dev.tiles, rt.tiles.data(), nt * sizeof(ScanTile), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(dev.wins, rt.wins.data(), nw * sizeof(WinDesc), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(dev.masks, p.mk.data(), p.mk.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(dev.n, p.nk.data(), p.nk.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    return IMPOP_OK;
}

template <int WPS>
static void launch_scan_fixed(impop_scan_plan *p, hipStream_t st) {
    MaskArgs<WPS> mk;
    for (int k = 0; k < WPS; ++k) {
        mk.p[k] = p->masks[k];
        mk.a[k] = p->masks[WPS + k];
        mk.b[k] = p->masks[2 * WPS + k];
    }
#define LAUNCH(SP, UQ)                                                                                                        \
    hipLaunchKernelGGL((scan_tiles_kernel<WPS, SP, UQ>), dim3((uint32_t)p->n_tiles), dim3(256), 0, st, p->sb, p->rare, p->d_tiles, \
                       mk, p->ps, p->d_parts, p->single, (const SingleRange *)p->d_singles, p->uniq, p->uniq_wt,                \
                       (const UniqRange *)p->d_uniqs)
#define LAUNCH_WAVE(SP)                                                                                                        \
    hipLaunchKernelGGL((scan_tiles_kernel_wave<WPS, SP>), dim3((uint32_t)((p->n_tiles + 3) / 4)), dim3(256), 0, st, p->sb, p->rare, \
                       p->d_tiles, mk, p->ps, p->d_parts, p->single, (const SingleRange *)p->d_singles, p->uniq, p->uniq_wt,    \
                       (const UniqRange *)p->d_uniqs, (uint32_t)p->n_tiles)
#define LAUNCH_DIGEST(SP)                                                                                                          \
    hipLaunchKernelGGL((scan_tiles_kernel_digest<WPS, SP>), dim3((uint32_t)((p->n_tiles + 3) / 4)), dim3(256), 0, st,                  \
                       (const uint32_t *)p->d_digest, (const uint16_t *)((const char *)p->d_digest + p->digest_weight_off),           \
                       (const uint16_t *)((const char *)p->d_digest + p->digest_hist_off), (const DigestDesc *)p->d_descs, p->rare, \
                       p->single, mk, p->ps, p->d_parts, (uint32_t)p->n_tiles)
    if (p->d_digest)     { if (p->subset_p) LAUNCH_DIGEST(true); else LAUNCH_DIGEST(false); }
    else if (p->wave_tiles) { if (p->subset_p) LAUNCH_WAVE(true); else LAUNCH_WAVE(false); }
    else if (p->d_uniqs) { if (p->subset_p) LAUNCH(true, true); else LAUNCH(false, true); }
    else                 { if (p->subset_p) LAUNCH(true, false); else LAUNCH(false, false); }
#undef LAUNCH_DIGEST
#undef LAUNCH_WAVE
#undef LAUNCH
}

IMPOP_API int impop_scan_plan_create(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows,
                                     uint64_t n_windows, const uint64_t *mask_p, const uint64_t *mask_a,
                                     const uint64_t *mask_b, const impop_scan_params *params, impop_scan_plan **out) {
    return scan_plan_create(ctx, m, windows, n_windows, mask_p, mask_a, mask_b, params, true, out);
}

int impop::scan_plan_create(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows,
                            const uint64_t *mask_p, const uint64_t *mask_a, const uint64_t *mask_b, const impop_scan_params *params,
                            bool reusable, impop_scan_plan **out) {
    REQUIRE(ctx && m && out, "impop_scan_plan_create: NULL argument");
    *out = nullptr;
    REQUIRE(n_windows == 0 || windows, "impop_scan_plan_create: windows is NULL");
    REQUIRE(m->device == ctx->device, "impop_scan_plan_create: matrix lives on device %d, context on %d", m->device,
            ctx->device);
    REQUIRE(m->g.n_hap <= 65535, "impop_scan: n_hap %u > 65535 not supported by the 32-bit per-site products",
            m->g.n_hap);
    impop_scan_params prm;
    prm.struct_size = sizeof prm; prm.d_pi_mode = 0; prm.s_scope = 0; prm.tile_blocks = 0;
    if (params) {
        REQUIRE(params->struct_size == sizeof prm, "impop_scan_params.struct_size %u != %zu", params->struct_size, sizeof prm);
        prm = *params;
    }
    REQUIRE(prm.d_pi_mode >= 0 && prm.d_pi_mode <= 2, "impop_scan_params.d_pi_mode must be 0..2");
    REQUIRE(prm.s_scope == 0 || prm.s_scope == 1, "impop_scan_params.s_scope must be 0 or 1");
    REQUIRE(prm.tile_blocks <= 4096, "impop_scan_params.tile_blocks too large");
    int rc = check_windows("impop_scan", m, windows, n_windows);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    ScanRoute rt;
    // the plan will launch the fixed-WPS kernel (impop_scan_plan_launch), the one reader of the singleton and distinct-row streams
    const bool fixed_wps = m->wt_prefix.empty() && m->g.wps <= 16;
    rc = scan_route("impop_scan", ctx, m, windows, n_windows, prm.tile_blocks, rt, fixed_wps, false);  // the trace line: below
    if (rc) return rc;
    impop_scan_plan *p = new impop_scan_plan();
    p->ctx = ctx; p->m = m; p->n_windows = n_windows;
    p->sb = rt.sb; p->rare = rt.rare; p->single = rt.single;
    p->uniq = rt.uniq; p->uniq_wt = rt.uniq_wt; p->wave_tiles = rt.wave_tiles;
    p->n_tiles = rt.tiles.size(); p->bytes_streamed = rt.bytes_streamed;
    m->users++;
    p->d_pi_mode = prm.d_pi_mode; p->s_scope = prm.s_scope;
    const uint32_t wps = m->g.wps;
    plan_set_masks(p, mask_p, mask_a, mask_b);
    uint64_t longest_range = 0;
    for (const WinDesc &w : rt.wins) longest_range = std::max(longest_range, w.t1 - w.t0);
    p->finalize_tpw = longest_range > 2048 ? 256 : longest_range > 48 ? 64 : 1;
    auto fail = [&](int code) {
        impop_scan_plan_destroy(p);
        return code;
    };
    hipError_t e;
#define PLAN_TRY(expr) \
    if ((e = (expr)) != hipSuccess) return fail(hip_fail(e, #expr, __FILE__, __LINE__))
    PLAN_TRY(hipMalloc((void **)&p->d_tiles, std::max<size_t>(rt.tiles.size(), 1) * sizeof(ScanTile)));
    PLAN_TRY(hipMalloc((void **)&p->d_parts, std::max<size_t>(rt.tiles.size(), 1) * sizeof(TilePartial)));
    PLAN_TRY(hipMalloc((void **)&p->d_wins, std::max<size_t>(n_windows, 1) * sizeof(WinDesc)));
    PLAN_TRY(hipMalloc((void **)&p->d_out, std::max<size_t>(n_windows, 1) * sizeof(impop_window_stats)));
    PLAN_TRY(hipMalloc((void **)&p->d_masks, (size_t)3 * wps * 4));
    PLAN_TRY(hipMalloc((void **)&p->d_taj, 8 * sizeof(double)));
    if ((rc = plan_fill_tajima(p))) return fail(rc);
    if (rt.packed) {
        PLAN_TRY(hipMalloc((void **)&p->d_singles, std::max<size_t>(rt.singles.size(), 1) * sizeof(SingleRange)));
        if (!rt.singles.empty()) PLAN_TRY(hipMemcpyAsync(p->d_singles, rt.singles.data(), rt.singles.size() * sizeof(SingleRange), hipMemcpyHostToDevice, ctx->stream));
    }
    if (rt.uniq) {
        PLAN_TRY(hipMalloc((void **)&p->d_uniqs, std::max<size_t>(rt.uniqs.size(), 1) * sizeof(UniqRange)));
        if (!rt.uniqs.empty()) PLAN_TRY(hipMemcpyAsync(p->d_uniqs, rt.uniqs.data(), rt.uniqs.size() * sizeof(UniqRange), hipMemcpyHostToDevice, ctx->stream));
    }
    if (!rt.tiles.empty()) PLAN_TRY(hipMemcpyAsync(p->d_tiles, rt.tiles.data(), rt.tiles.size() * sizeof(ScanTile), hipMemcpyHostToDevice, ctx->stream));
    if (n_windows) PLAN_TRY(hipMemcpyAsync(p->d_wins, rt.wins.data(), n_windows * sizeof(WinDesc), hipMemcpyHostToDevice, ctx->stream));
    PLAN_TRY(hipMemcpyAsync(p->d_masks, p->masks.data(), (size_t)3 * wps * 4, hipMemcpyHostToDevice, ctx->stream));
    // the tile digest, where the plan takes one: built behind the uploads it reads, and the plan then reports what its launches read
    if ((rc = plan_build_digest(p, rt, reusable))) return fail(rc);
    p->bytes_streamed = rt.bytes_streamed;
    trace_route(m, rt, n_windows);
    PLAN_TRY(hipStreamSynchronize(ctx->stream));  // host vectors die at return
#undef PLAN_TRY
    *out = p;
    return IMPOP_OK;
}

IMPOP_API int impop_scan_plan_set_masks(impop_scan_plan *p, const uint64_t *mask_p, const uint64_t *mask_a,
                                        const uint64_t *mask_b) {
    REQUIRE(p, "impop_scan_plan_set_masks: plan is NULL");
    HIP_TRY(hipSetDevice(p->ctx->device));
    // launches already queued read the previous masks: kernel arguments were captured at their launch and
    // the device copy is only rewritten behind them in stream order
    plan_set_masks(p, mask_p, mask_a, mask_b);
    HIP_TRY(hipMemcpyAsync(p->d_masks, p->masks.data(), p->masks.size() * 4, hipMemcpyHostToDevice, p->ctx->stream));
    // ... and so are the plan's Tajima constants where nP changed.  A graph captured before holds the previous subset sizes
    // and kernel choice as arguments of its launches: capture again after this call
    return plan_fill_tajima(p);
}

IMPOP_API int impop_scan_plan_launch(impop_scan_plan *p, void *d_out) {
    REQUIRE(p, "impop_scan_plan_launch: plan is NULL");
    impop_ctx *ctx = p->ctx;
    hipStream_t st = ctx->stream;
    // one process may drive several devices (impop_scan_sharded): kernels go to the device the plan's stream lives on
    HIP_TRY(hipSetDevice(ctx->device));
    // exactly the two kernels below, on the plan's own buffers (its Tajima constants too: p->d_taj): nothing of the context
    // is read or written, so what a capture records and what its replay runs cannot disagree
    int rc = IMPOP_OK;
    const bool timed = p->timing && p->n_tiles;
    size_t slot = 0;
    if (timed && (rc = p->timer.begin(st, &slot))) return rc;
    const bool weighted = !p->m->wt_prefix.empty();  // W of each window came from the host prefix sums at plan time
    const uint32_t wps = p->m->g.wps;
    if (p->n_tiles && (weighted || wps > 16)) {
        const size_t lds = (size_t)3 * ((wps + 3) & ~3u) * 4;
#define ANYN(SP, WT)                                                                                                     \
    hipLaunchKernelGGL((scan_tiles_anyn_kernel<SP, WT>), dim3((uint32_t)p->n_tiles), dim3(256), lds, st, p->sb, p->rare, \
                       p->d_tiles, p->d_masks, wps, p->m->g.G, p->m->g.r, p->ps, p->m->d_wt, p->d_parts)
        if (weighted) { if (p->subset_p) ANYN(true, true); else ANYN(false, true); }
        else          { if (p->subset_p) ANYN(true, false); else ANYN(false, false); }
#undef ANYN
        HIP_TRY(hipGetLastError());
    } else if (p->n_tiles) {
        switch (wps) {
#define CASE(W) case W: launch_scan_fixed<W>(p, st); break;
            CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)
            CASE(9) CASE(10) CASE(11) CASE(12) CASE(13) CASE(14) CASE(15) CASE(16)
#undef CASE
        }
        HIP_TRY(hipGetLastError());
    }
    if (timed && (rc = p->timer.end(st, slot))) return rc;
    if (p->n_windows) {
        impop_window_stats *dst = d_out ? (impop_window_stats *)d_out : p->d_out;
        if (p->finalize_tpw == 1)
            hipLaunchKernelGGL(scan_finalize_kernel<1>, dim3((uint32_t)((p->n_windows + 127) / 128)), dim3(128), 0, st, p->d_parts,
                               p->d_wins, p->n_windows, p->ps, p->d_taj, p->d_pi_mode, p->s_scope, dst);
        else if (p->finalize_tpw == 64)
            hipLaunchKernelGGL(scan_finalize_kernel<64>, dim3((uint32_t)((p->n_windows + 3) / 4)), dim3(256), 0, st, p->d_parts,
                               p->d_wins, p->n_windows, p->ps, p->d_taj, p->d_pi_mode, p->s_scope, dst);
        else
            hipLaunchKernelGGL(scan_finalize_kernel<256>, dim3((uint32_t)p->n_windows), dim3(256), 0, st, p->d_parts,
                               p->d_wins, p->n_windows, p->ps, p->d_taj, p->d_pi_mode, p->s_scope, dst);
        HIP_TRY(hipGetLastError());
    }
    return IMPOP_OK;
}

IMPOP_API int impop_scan_plan_fetch(impop_scan_plan *p, impop_window_stats *out_host) {
    REQUIRE(p && (out_host || p->n_windows == 0), "impop_scan_plan_fetch: NULL argument");
    HIP_TRY(hipSetDevice(p->ctx->device));
    if (p->n_windows)
        HIP_TRY(hipMemcpyAsync(out_host, p->d_out, p->n_windows * sizeof(impop_window_stats), hipMemcpyDeviceToHost,
                               p->ctx->stream));
    HIP_TRY(hipStreamSynchronize(p->ctx->stream));
    return IMPOP_OK;
}

IMPOP_API int impop_scan_plan_device_records(impop_scan_plan *p, void **d_records) {
    REQUIRE(p && d_records, "impop_scan_plan_device_records: NULL argument");
    *d_records = p->d_out;
    return IMPOP_OK;
}

IMPOP_API int impop_scan_plan_info(const impop_scan_plan *p, uint64_t *n_tiles, uint64_t *bytes_streamed) {
    REQUIRE(p, "impop_scan_plan_info: plan is NULL");
    if (n_tiles) *n_tiles = p->n_tiles;
    if (bytes_streamed) *bytes_streamed = p->bytes_streamed;
    return IMPOP_OK;
}

IMPOP_API int impop_scan_plan_digest_info(const impop_scan_plan *p, int *on, uint64_t *n_rows, uint64_t *n_hist_tiles,
                                          uint64_t *digest_bytes, char *why, size_t why_len) {
    REQUIRE(p, "impop_scan_plan_digest_info: plan is NULL");
    if (on) *on = p->d_digest != nullptr;
    if (n_rows) *n_rows = p->digest_rows;
    if (n_hist_tiles) *n_hist_tiles = p->digest_hist_tiles;
    if (digest_bytes) *digest_bytes = p->digest_bytes;
    if (why && why_len) snprintf(why, why_len, "%s", p->digest_why.c_str());
    return IMPOP_OK;
}

IMPOP_API int impop_scan_plan_timing(impop_scan_plan *p, int enable) {
    REQUIRE(p, "impop_scan_plan_timing: plan is NULL");
    HIP_TRY(hipSetDevice(p->ctx->device));
    HIP_TRY(hipStreamSynchronize(p->ctx->stream));
    p->timing = enable != 0;
    p->timer.reset();
    return IMPOP_OK;
}

IMPOP_API int impop_scan_plan_elapsed(impop_scan_plan *p, double *total_ms, uint64_t *launches) {
    REQUIRE(p, "impop_scan_plan_elapsed: plan is NULL");
    HIP_TRY(hipSetDevice(p->ctx->device));
    HIP_TRY(hipStreamSynchronize(p->ctx->stream));
    return p->timer.elapsed(total_ms, launches);
}

IMPOP_API int impop_debug_timer_pool_sizes(const impop_ctx *ctx, const impop_scan_plan *plan, uint64_t sizes[4]) {
    REQUIRE(ctx && sizes, "impop_debug_timer_pool_sizes: NULL argument");
    sizes[0] = ctx->timers[impop_ctx::T_GRAM].pool.size();
    sizes[1] = ctx->timers[impop_ctx::T_CLUSTER].pool.size();
    sizes[2] = ctx->timers[impop_ctx::T_EHH].pool.size();
    sizes[3] = plan ? plan->timer.pool.size() : 0;
    return IMPOP_OK;
}

IMPOP_API int impop_scan_plan_destroy(impop_scan_plan *p) {
    if (!p) return IMPOP_OK;
    hipSetDevice(p->ctx->device);
    hipStreamSynchronize(p->ctx->stream);
    p->timer.destroy();
    if (p->d_tiles) hipFree(p->d_tiles);
    if (p->d_parts) hipFree(p->d_parts);
    if (p->d_wins) hipFree(p->d_wins);
    if (p->d_out) hipFree(p->d_out);
    if (p->d_masks) hipFree(p->d_masks);
    if (p->d_taj) hipFree(p->d_taj);
    if (p->d_singles) hipFree(p->d_singles);
    if (p->d_uniqs) hipFree(p->d_uniqs);
    if (p->d_digest) hipFree(p->d_digest);
    if (p->d_descs) hipFree(p->d_descs);
    if (p->m) p->m->users--;
    delete p;
    return IMPOP_OK;
}

IMPOP_API int impop_scan(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows,
                         const uint64_t *mask_p, const uint64_t *mask_a, const uint64_t *mask_b,
                         const impop_scan_params *params, impop_window_stats *out_host) {
    impop_scan_plan *p = nullptr;
    int rc = scan_plan_create(ctx, m, windows, n_windows, mask_p, mask_a, mask_b, params, false, &p);
    if (rc) return rc;
    rc = impop_scan_plan_launch(p, nullptr);
    if (!rc) rc = impop_scan_plan_fetch(p, out_host);
    impop_scan_plan_destroy(p);
    return rc;
}

IMPOP_API int impop_site_counts(impop_ctx *ctx, const impop_matrix *m, const uint64_t *mask, uint64_t site_begin,
                                uint64_t site_end, uint32_t *out_host) {
    REQUIRE(ctx && m, "impop_site_counts: NULL argument");
    NOT_COMPACT(m, "impop_site_counts");
    REQUIRE(site_begin <= site_end && site_end <= m->g.n_site, "impop_site_counts: bad site range");
    const uint64_t W = site_end - site_begin;
    if (!W) return IMPOP_OK;
    REQUIRE(out_host, "impop_site_counts: out is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    std::vector<uint32_t> mk;
    mask_to_dwords(mask, m->g.n_hap, m->g.wps, true, mk);
    void *d = nullptr;
    Carve L;
    const size_t o_mask = L.take<uint32_t>(m->g.wps), o_cnt = L.take<uint32_t>(W);
    int rc = ctx_scratch(ctx, L.total(), &d);
    if (rc) return rc;
    uint32_t *d_mask = L.at<uint32_t>(d, o_mask), *d_cnt = L.at<uint32_t>(d, o_cnt);
    HIP_TRY(hipMemcpyAsync(d_mask, mk.data(), (size_t)m->g.wps * 4, hipMemcpyHostToDevice, ctx->stream));
    const uint64_t nb = (site_end + 63) / 64 - site_begin / 64;
    REQUIRE((nb + 3) / 4 < 0x7FFFFFFFull, "impop_site_counts: range too long");
    hipLaunchKernelGGL(site_counts_kernel, dim3((uint32_t)((nb + 3) / 4)), dim3(256), 0, ctx->stream, m->d_sb, d_mask,
                       m->g.wps, m->g.G, m->g.r, site_begin, site_end, d_cnt);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out_host, d_cnt, W * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return IMPOP_OK;
}

IMPOP_API int impop_scan_multi(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows,
                               const uint64_t *masks, uint32_t n_pop, impop_pair_stats *out_host) {
    REQUIRE(ctx && m, "impop_scan_multi: NULL argument");
    REQUIRE(n_pop >= 2 && n_pop <= 8, "impop_scan_multi: n_pop must be 2..8");
    REQUIRE(masks, "impop_scan_multi: masks is NULL");
    REQUIRE(m->g.n_hap <= 65535, "impop_scan_multi: n_hap > 65535 not supported");
    if (!n_windows) return IMPOP_OK;
    REQUIRE(windows && out_host, "impop_scan_multi: NULL windows/out");
    int rc = check_windows("impop_scan_multi", m, windows, n_windows);
    if (rc) return rc;
    const uint32_t n = m->g.n_hap, wps = m->g.wps, K = n_pop, NP = K * (K - 1) / 2;
    PopPanel panel;
    pop_panel_pack(m, masks, K, panel);
    std::vector<uint32_t> seen(wps, 0u);
    for (uint32_t k = 0; k < K; ++k)
        for (uint32_t j = 0; j < wps; ++j) {
            // h-fst.py:181-185 removes shared members per pair; with K populations that would make
            // n_k pair-dependent, so the one-pass form requires disjoint populations
            REQUIRE((seen[j] & panel.mk[(size_t)k * wps + j]) == 0,
                    "impop_scan_multi: populations must be disjoint (population %u overlaps an earlier one)", k);
            seen[j] |= panel.mk[(size_t)k * wps + j];
        }
    HIP_TRY(hipSetDevice(ctx->device));
    ScanRoute rt;
    rc = scan_route("impop_scan_multi", ctx, m, windows, n_windows, 0, rt);
    if (rc) return rc;
    const size_t nt = rt.tiles.size();
    const uint64_t items = n_windows * NP;
    PopPanelDev dev;
    uint64_t *d_parts = nullptr;
    impop_pair_stats *d_out = nullptr;
    rc = pop_panel_upload(ctx, rt, panel, dev, [&](Layout &L) {
        L.sub(d_parts, std::max<size_t>(nt, 1) * (K + NP));
        L.sub(d_out, items);
    });
    if (rc) return rc;
    if (nt) {
        // 32-bit per-lane partial sums: unweighted, <= 512 haplotypes, <= 1024 sites per lane and tile
        const bool small = m->wt_prefix.empty() && n <= 512 && rt.tile_blocks <= 4096;
        rc = pop_dispatch_k<2>(K, [&](auto k) {
            return small ? pop_launch(scan_multi_kernel<k.value, true>, K, ctx->stream, m, rt, dev, m->d_wt, d_parts)
                         : pop_launch(scan_multi_kernel<k.value, false>, K, ctx->stream, m, rt, dev, m->d_wt, d_parts);
        });
        if (rc) return rc;
    }
    hipLaunchKernelGGL(scan_multi_finalize_kernel, dim3((uint32_t)((items + 127) / 128)), dim3(128), 0, ctx->stream,
                       (const uint64_t *)d_parts, (const WinDesc *)dev.wins, n_windows, K, (const uint32_t *)dev.n, d_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out_host, d_out, items * sizeof(impop_pair_stats), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return IMPOP_OK;
}

IMPOP_API int impop_afs(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows,
                        const uint64_t *mask, uint32_t *out_host) {
    REQUIRE(ctx && m, "impop_afs: NULL argument");
    NOT_COMPACT(m, "impop_afs");
    if (!n_windows) return IMPOP_OK;
    REQUIRE(windows && out_host, "impop_afs: NULL windows/out");
    uint64_t longest = 0;
    for (uint64_t i = 0; i < n_windows; ++i) {
        REQUIRE(windows[i].site_begin <= windows[i].site_end && windows[i].site_end <= m->g.n_site,
                "impop_afs: window %llu: bad site range", (unsigned long long)i);
        longest = std::max(longest, windows[i].site_end - windows[i].site_begin);
    }
    std::vector<uint32_t> mk;
    mask_to_dwords(mask, m->g.n_hap, m->g.wps, true, mk);
    const uint32_t bins = popcount_vec(mk) + 1;
    REQUIRE((size_t)bins * 4 <= 64 * 1024, "impop_afs: more than 16383 haplotypes in the mask");
    HIP_TRY(hipSetDevice(ctx->device));
    Carve L;
    const size_t o_mask = L.take<uint32_t>(m->g.wps), o_wins = L.take<impop_window>(n_windows),
                 o_out = L.take<uint32_t>(n_windows * bins);
    void *d = nullptr;
    int rc = ctx_scratch(ctx, L.total(), &d);
    if (rc) return rc;
    char *base = (char *)d;
    HIP_TRY(hipMemcpyAsync(base + o_mask, mk.data(), (size_t)m->g.wps * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(base + o_wins, windows, n_windows * sizeof(impop_window), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemsetAsync(base + o_out, 0, n_windows * bins * 4, ctx->stream));
    // a workgroup per window when there are thousands of them (one flush of the histogram per window, no atomics), more —
    // never shorter than 4096 sites — when few windows would leave CUs idle (about 32 workgroups per CU wanted)
    const uint64_t want = 32ull * (uint64_t)(ctx->n_cu > 0 ? ctx->n_cu : 256);
    uint64_t chunks = std::min<uint64_t>((longest + 4095) / 4096, std::max<uint64_t>(1, (want + n_windows - 1) / std::max<uint64_t>(n_windows, 1)));
    const uint64_t chunk_sites = chunks ? ((longest + chunks - 1) / chunks + 63) / 64 * 64 : 0;
    if (chunks) chunks = (longest + chunk_sites - 1) / chunk_sites;
    if (chunks) {
        REQUIRE(chunks < 0x7FFFFFFFull, "impop_afs: window too long");
        if ((rc = lds_opt_in(afs_kernel, (size_t)bins * 4))) return rc;  // 12288 .. 16383 haplotypes in the mask
        // windows ride on gridDim.y (<= 65535): any number of windows goes out in batches of that many
        for (uint64_t w0 = 0; w0 < n_windows; w0 += 65535) {
            const uint32_t nw = (uint32_t)std::min<uint64_t>(65535, n_windows - w0);
            hipLaunchKernelGGL(afs_kernel, dim3((uint32_t)chunks, nw), dim3(256), (size_t)bins * 4, ctx->stream, m->d_sb,
                               (const uint32_t *)(base + o_mask), m->g.wps, m->g.G, m->g.r,
                               (const impop_window *)(base + o_wins) + w0, bins, chunk_sites, (uint32_t *)(base + o_out) + w0 * bins);
            HIP_TRY(hipGetLastError());
        }
    }
    HIP_TRY(hipMemcpyAsync(out_host, base + o_out, n_windows * bins * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return IMPOP_OK;
}
