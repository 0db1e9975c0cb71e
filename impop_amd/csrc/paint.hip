// paint.hip — impop_paint_scan: every recipient haplotype as a Viterbi mosaic of donor haplotypes (include/impop_hip.h).
//
// The operand is the word-major transposed stream of ibs_transpose.h, [64-site block][row] uint64, rows = the donors and the
// recipients, made per chunk of blocks.  The arithmetic is csrc/paint_math.h; nothing of it is restated here.
//   forward    one wave per recipient, its states in registers: slot k = q * 64 + lane, Q = 1, 2, 4, 8 or 16 slots per lane.  Per
//              64-site block a lane loads its Q donor words once and XORs them with the recipient's (wave-uniform) word: 64 sites
//              of mismatch bits.  Per site: Q state updates, the lane's smallest packed word, ONE wave minimum in the VALU (DPP),
//              the origin of the winning state by readlane, the renormalisation.  The site's record (A(s), T(s)) stays in the
//              register of lane s & 63 and the block's 64 records leave in one coalesced store.  No LDS, no barrier, no atomic.
//              States and the 64-bit cost are carried between site chunks in scratch.
//   count      one thread per recipient walks the records backwards, one jump per segment -> n_segments.  The host prefixes them.
//   emit       the same walk writes the segments at the recipient's offset, last first; a segment the count did not announce is
//              not written and sets the device error word.
//   mismatch   one wave per segment and site chunk: popcount of (donor word ^ recipient word) over the segment's sites.
//   windows    one wave per (window, recipient): the overlapping segments by binary search; cells by panel, switches, mismatches.
//   records    one wave per recipient: sums, the longest segment, the two chunk matrices, and the self-check
//              mu * n_mismatch + sum of c_s over the switches == the forward pass's cost, sum of n_sites == L.
// Recipients run in ranges whose records fit half the budget.  With one site chunk the words are transposed once for the call;
// with several, every range transposes them for the forward pass and again for the mismatch and window kernels.
// Every loop is bounded by a count from the host (blocks of the chunk, L, announced segments); no spin waits.
#include <string.h>

#include <algorithm>
#include <vector>

#include "chunk_run.h"
#include "device_utils.h"
#include "ibs_transpose.h"
#include "internal.h"
#include "paint_math.h"
#include "scan_route.h"
#include "win_chunks.h"

namespace impop {

static_assert(PAINT_MAX_DONORS == IMPOP_PAINT_MAX_DONORS && PAINT_MAX_RECIPIENTS == IMPOP_PAINT_MAX_RECIPIENTS &&
                  PAINT_MAX_PANELS == IMPOP_PAINT_MAX_PANELS && PAINT_MAX_COST == IMPOP_PAINT_MAX_COST,
              "paint_math.h states the public limits");
static_assert(sizeof(PaintRec) == 8, "the per-site record is 8 bytes");
constexpr uint32_t PAINT_NO_PANEL_SLOT = 8;

struct PaintArgs {
    const uint64_t *wm;        // the chunk's words
    const uint64_t *pos;       // compacted: the kept sites' original coordinates, else null
    const uint32_t *csw;       // c_s per site of the range, or null: the constant
    const int32_t *ppos;       // haplotype -> row
    const uint32_t *rows;      // row -> haplotype
    const uint32_t *rrow, *rhap, *ndon;  // per recipient: its row, its haplotype, its admissible donors
    const uint32_t *drow;      // [recipient][dstride]: slot -> row
    const uint8_t *pslot;      // haplotype -> panel slot 0..8
    PaintRec *rec;             // [recipient of the range][L]
    uint32_t *stR, *stT;       // [recipient of the range][Q][64]: the states between site chunks
    unsigned long long *cost;  // [recipient]
    uint32_t *nseg;            // [recipient]
    const uint64_t *off;       // [recipient of the range + 1]: offsets into the staging
    impop_paint_segment *seg;  // the range's segments
    uint32_t *seg_s0;          // and their first stored sites
    uint32_t *cc;              // [recipient of the range][n_hap]
    unsigned long long *cs;
    impop_paint_recipient *out;  // [recipient]
    impop_paint_window *win;   // [window]
    const uint32_t *wlo, *whi; // the windows' stored-site ranges inside the range
    uint32_t *anc;             // [window][recipient][np1], or null
    uint32_t *err;
    uint64_t b, e, cb, blk_abs0, len;  // the range (original coordinates), its first column, the chunk's first block and blocks
    uint32_t L, stride, dstride, r0, r1, n_rec, n_hap, mu, cconst, np1, n_win;
};

__device__ inline uint32_t paint_cost_at(const PaintArgs &A, uint32_t s) { return s == 0 ? 0u : A.csw ? A.csw[s] : A.cconst; }
__device__ inline uint64_t paint_coord(const PaintArgs &A, uint32_t s) { return A.pos ? A.pos[A.cb + s] : A.cb + s; }

// the chunk's stored sites [lo, hi), relative to the range
__device__ inline void paint_chunk_sites(const PaintArgs &A, uint32_t &lo, uint32_t &hi) {
    const uint64_t c0 = A.blk_abs0 * 64, c1 = (A.blk_abs0 + A.len) * 64, ce = A.cb + A.L;
    lo = (uint32_t)((c0 > A.cb ? c0 : A.cb) - A.cb);
    hi = (uint32_t)((c1 < ce ? c1 : ce) - A.cb);
}

// sites of [lo, hi) (inside the chunk) where rows ra and rb differ: this lane's share, the blocks lane, lane + 64, ..
__device__ inline uint32_t paint_mismatches(const PaintArgs &A, uint32_t ra, uint32_t rb, uint32_t lo, uint32_t hi, uint32_t lane) {
    const uint64_t c0 = A.cb + lo, c1 = A.cb + hi;
    uint32_t n = 0;
    for (uint64_t blk = (c0 >> 6) + lane; blk < ((c1 + 63) >> 6); blk += 64) {
        const uint64_t *w = A.wm + (blk - A.blk_abs0) * A.stride;
        uint64_t x = w[ra] ^ w[rb];
        if (blk * 64 < c0) x &= ~0ull << (c0 - blk * 64);
        if (c1 - blk * 64 < 64) x &= (1ull << (c1 - blk * 64)) - 1ull;
        n += (uint32_t)__builtin_popcountll(x);
    }
    return n;
}

// grid = recipients of the range, one wave each.  first: the chunk holds site 0, the states start empty
template <int Q>
__global__ __launch_bounds__(64) void paint_forward_kernel(const PaintArgs A, int first) {
    const uint32_t lane = threadIdx.x, rl = blockIdx.x, r = A.r0 + rl;
    const uint32_t nd = A.ndon[r], rrow = A.rrow[r], mu = A.mu;
    uint32_t R[Q], T[Q], row[Q];
    bool act[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const uint32_t slot = (uint32_t)q * 64u + lane;
        act[q] = slot < nd;
        row[q] = act[q] ? A.drow[(uint64_t)r * A.dstride + slot] : rrow;
        R[q] = first ? 0u : A.stR[((uint64_t)rl * Q + q) * 64 + lane];
        T[q] = first ? 0u : A.stT[((uint64_t)rl * Q + q) * 64 + lane];
    }
    uint64_t cost = first ? 0ull : A.cost[r];
    PaintRec *rec = A.rec + (uint64_t)rl * A.L;
    const uint64_t ce = A.cb + A.L;
    for (uint64_t bi = 0; bi < A.len; ++bi) {
        const uint64_t col0 = (A.blk_abs0 + bi) * 64;
        const uint32_t t_lo = col0 < A.cb ? (uint32_t)(A.cb - col0) : 0u, t_hi = ce - col0 < 64 ? (uint32_t)(ce - col0) : 64u;
        const uint64_t *w = A.wm + bi * A.stride;
        const uint64_t xr = w[rrow];
        uint64_t x[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) x[q] = w[row[q]] ^ xr;
        const bool mine = lane >= t_lo && lane < t_hi;  // lane t holds site t's cost and, afterwards, its record
        const uint32_t s_mine = (uint32_t)(col0 + lane - A.cb);
        const uint32_t c_mine = mine ? paint_cost_at(A, s_mine) : 0u;
        PaintRec keep{0u, 0u};
        for (uint32_t half = 0; half < 2; ++half) {
            uint32_t xh[Q];
#pragma unroll
            for (int q = 0; q < Q; ++q) xh[q] = half ? (uint32_t)(x[q] >> 32) : (uint32_t)x[q];
            const uint32_t ta = t_lo > 32 * half ? t_lo : 32 * half, tb = t_hi < 32 * half + 32 ? t_hi : 32 * half + 32;
            for (uint32_t t = ta; t < tb; ++t) {  // wave-uniform
                const uint32_t s = (uint32_t)(col0 + t - A.cb);
                const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)c_mine, (int)t);
                uint32_t best = 0xFFFFFFFFu, best_org = 0u;
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    paint_site_update(R[q], T[q], c, (xh[q] >> (t & 31u)) & 1u, mu, s);
                    R[q] = act[q] ? R[q] : PAINT_IDLE;
                    const uint32_t p = paint_pack(R[q], (uint32_t)q * 64u + lane);
                    best_org = p < best ? T[q] : best_org;
                    best = p < best ? p : best;
                }
                const uint32_t m = (uint32_t)__builtin_amdgcn_readlane((int)wave_min_u32_dpp(best), 63);
                const uint32_t site_min = paint_pack_value(m), a = paint_pack_slot(m);
                const uint32_t org = (uint32_t)__builtin_amdgcn_readlane((int)best_org, (int)(a & 63u));
                if (lane == t) keep = PaintRec{a, org};
                cost += site_min;
#pragma unroll
                for (int q = 0; q < Q; ++q) paint_renorm(R[q], site_min);
            }
        }
        if (mine) rec[s_mine] = keep;
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        A.stR[((uint64_t)rl * Q + q) * 64 + lane] = R[q];
        A.stT[((uint64_t)rl * Q + q) * 64 + lane] = T[q];
    }
    if (lane == 0) A.cost[r] = cost;
}

// grid = ceil(recipients of the range / 64): a thread per recipient.  emit == 0: n_segments; else the segments, last first
__global__ __launch_bounds__(64) void paint_backtrack_kernel(const PaintArgs A, int emit) {
    const uint32_t rl = blockIdx.x * 64 + threadIdx.x, r = A.r0 + rl;
    if (r >= A.r1) return;
    const PaintRec *rec = A.rec + (uint64_t)rl * A.L;
    if (!emit) {
        A.nseg[r] = paint_backtrack(rec, A.L, A.L, [](uint32_t, uint32_t, uint32_t, uint32_t) {});
        return;
    }
    const uint32_t announced = A.nseg[r], nd = A.ndon[r], h = A.rhap[r];
    const uint64_t base = A.off[rl];
    bool bad = false;
    const uint32_t n = paint_backtrack(rec, A.L, announced, [&](uint32_t k, uint32_t slot, uint32_t s0, uint32_t s1) {
        if (slot >= nd) {
            bad = true;
            slot = 0;
        }
        impop_paint_segment o;
        o.h = h;
        o.donor = A.rows[A.drow[(uint64_t)r * A.dstride + slot]];
        o.begin = s0 == 0 ? A.b : paint_coord(A, s0);
        o.end = s1 == A.L ? A.e : paint_coord(A, s1);
        o.n_sites = s1 - s0;
        o.n_mismatch = 0;
        o.recipient = r;
        o.reserved = 0;
        const uint64_t i = base + (announced - 1u - k);  // k < announced: the walk's bound
        A.seg[i] = o;
        A.seg_s0[i] = s0;
    });
    if (bad || n != announced) atomicOr(A.err, DEV_ERR_PAINT);
}

// grid = ceil(segments of the range / 4): a wave per segment adds its mismatches inside the chunk
__global__ __launch_bounds__(256) void paint_mismatch_kernel(const PaintArgs A, uint64_t n_seg) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t g = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= n_seg) return;  // wave-uniform
    uint32_t clo, chi;
    paint_chunk_sites(A, clo, chi);
    const uint32_t s0 = A.seg_s0[g], s1 = s0 + A.seg[g].n_sites;
    const uint32_t lo = s0 > clo ? s0 : clo, hi = s1 < chi ? s1 : chi;
    if (lo >= hi) return;
    const int32_t dr = A.ppos[A.seg[g].donor];
    const uint32_t n = wave_sum_u32(paint_mismatches(A, A.rrow[A.seg[g].recipient], (uint32_t)dr, lo, hi, lane));
    if (lane == 0) A.seg[g].n_mismatch += n;
}

// grid = windows x recipients of the range, a wave each.  cells: also the quantities that do not depend on the words (once per range)
__global__ __launch_bounds__(64) void paint_window_kernel(const PaintArgs A, int cells) {
    const uint32_t lane = threadIdx.x, nr = A.r1 - A.r0;
    const uint32_t wi = blockIdx.x / nr, rl = blockIdx.x % nr, r = A.r0 + rl;
    const uint32_t wlo = A.wlo[wi], whi = A.whi[wi];
    if (whi <= wlo) return;
    uint32_t clo, chi;
    paint_chunk_sites(A, clo, chi);
    const uint64_t base = A.off[rl];
    const uint32_t n = (uint32_t)(A.off[rl + 1] - base), rrow = A.rrow[r];
    // the last segment that begins at or left of wlo (segment 0 begins at site 0)
    uint32_t k = 0, top = n;
    while (top - k > 1) {  // at most 32 rounds
        const uint32_t mid = k + (top - k) / 2;
        if (A.seg_s0[base + mid] <= wlo) k = mid;
        else top = mid;
    }
    uint32_t mm = 0, copied = 0, sw = 0;
    for (; k < n; ++k) {
        const uint32_t s0 = A.seg_s0[base + k];
        if (s0 >= whi) break;
        const impop_paint_segment sg = A.seg[base + k];
        const uint32_t s1 = s0 + sg.n_sites;
        if (cells) {
            if (lane == A.pslot[sg.donor]) copied += paint_overlap(s0, s1, wlo, whi);
            sw += (s0 >= 1 && s0 >= wlo) ? 1u : 0u;
        }
        const uint32_t lo = (s0 > wlo ? s0 : wlo) > clo ? (s0 > wlo ? s0 : wlo) : clo, hi = (s1 < whi ? s1 : whi) < chi ? (s1 < whi ? s1 : whi) : chi;
        if (lo < hi) mm += paint_mismatches(A, rrow, (uint32_t)A.ppos[sg.donor], lo, hi, lane);
    }
    mm = wave_sum_u32(mm);
    if (lane == 0 && mm) atomicAdd((unsigned long long *)&A.win[wi].n_mismatch, (unsigned long long)mm);
    if (!cells) return;
    if (lane <= PAINT_NO_PANEL_SLOT) {
        if (copied) atomicAdd((unsigned long long *)&A.win[wi].copied[lane], (unsigned long long)copied);
        const uint32_t slot = lane == PAINT_NO_PANEL_SLOT ? A.np1 - 1u : lane;
        if (A.anc && (lane == PAINT_NO_PANEL_SLOT || lane < A.np1 - 1u)) A.anc[((uint64_t)wi * A.n_rec + r) * A.np1 + slot] = copied;
    }
    if (lane == 0) {
        if (sw) atomicAdd((unsigned long long *)&A.win[wi].n_switches, (unsigned long long)sw);
        atomicAdd((unsigned long long *)&A.win[wi].cells, (unsigned long long)(whi - wlo));
    }
}

__device__ inline uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

// grid = recipients of the range, a wave each: the recipient's record, its rows of the two chunk matrices, the self-check
__global__ __launch_bounds__(64) void paint_record_kernel(const PaintArgs A) {
    const uint32_t lane = threadIdx.x, rl = blockIdx.x, r = A.r0 + rl;
    const uint64_t base = A.off[rl];
    const uint32_t n = (uint32_t)(A.off[rl + 1] - base);
    uint64_t mm = 0, sites = 0, sw = 0, longest = 0;
    uint32_t distinct = 0;
    for (uint32_t k = lane; k < n; k += 64) {
        const impop_paint_segment sg = A.seg[base + k];
        const uint32_t s0 = A.seg_s0[base + k];
        mm += sg.n_mismatch;
        sites += sg.n_sites;
        sw += paint_cost_at(A, s0);
        const uint64_t key = ((uint64_t)sg.n_sites << 32) | (0xFFFFFFFFu - k);  // the longest, the first of equals
        longest = key > longest ? key : longest;
        distinct += atomicAdd(&A.cc[(uint64_t)rl * A.n_hap + sg.donor], 1u) == 0u ? 1u : 0u;
        atomicAdd(&A.cs[(uint64_t)rl * A.n_hap + sg.donor], (unsigned long long)sg.n_sites);
    }
    mm = wave_sum_u64(mm);
    sites = wave_sum_u64(sites);
    sw = wave_sum_u64(sw);
    longest = wave_max_u64(longest);
    distinct = wave_sum_u32(distinct);
    if (lane != 0) return;
    const uint64_t cost = A.cost[r];
    if ((uint64_t)A.mu * mm + sw != cost || sites != A.L || n != A.nseg[r]) atomicOr(A.err, DEV_ERR_PAINT);
    impop_paint_recipient o;
    o.h = A.rhap[r];
    o.n_donors = A.ndon[r];
    o.n_segments = n;
    o.n_mismatch = (uint32_t)mm;
    o.distinct_donors = distinct;
    o.longest_sites = (uint32_t)(longest >> 32);
    o.longest_donor = n ? A.seg[base + (0xFFFFFFFFu - (uint32_t)longest)].donor : 0u;
    o.reserved = 0;
    o.cost = cost;
    A.out[r] = o;
}

template <int Q>
static void paint_launch_forward(impop_ctx *ctx, const PaintArgs &A, int first) {
    hipLaunchKernelGGL(paint_forward_kernel<Q>, dim3(A.r1 - A.r0), dim3(64), 0, ctx->stream, A, first);
}

}  // namespace impop

using namespace impop;

IMPOP_API int impop_paint_scan(impop_ctx *ctx, const impop_matrix *m, const uint64_t *mask_d, const uint32_t *recipients, uint32_t n_rec,
                               const impop_window *windows, uint64_t n_windows, const impop_paint_params *params,
                               impop_paint_recipient *rec_out, impop_paint_segment *seg_out, uint64_t seg_capacity, uint64_t *n_segments,
                               uint32_t *chunk_counts, uint64_t *chunk_sites, impop_paint_window *win_out, uint32_t *anc_out) {
    static_assert(sizeof(impop_paint_params) == 72 && sizeof(impop_paint_recipient) == 40 && sizeof(impop_paint_segment) == 40 &&
                      sizeof(impop_paint_window) == 96,
                  "ABI layout");
    const char *fn = "impop_paint_scan";
    REQUIRE(ctx && m && params && n_segments && recipients, "%s: NULL argument", fn);
    REQUIRE(params->struct_size == sizeof(impop_paint_params), "impop_paint_params.struct_size mismatch");
    REQUIRE(m->device == ctx->device, "%s: matrix lives on device %d, context on %d", fn, m->device, ctx->device);
    const uint64_t span = matrix_span(m), b = params->site_begin, e = params->site_end ? params->site_end : span;
    REQUIRE(b < e && e <= span, "%s: bad range [%llu,%llu) for %llu sites", fn, (unsigned long long)b, (unsigned long long)e,
            (unsigned long long)span);
    REQUIRE(e - b < (1ull << 32), "%s: a range of %llu sites does not fit the records' 32-bit lengths", fn, (unsigned long long)(e - b));
    REQUIRE(windows || (!win_out && !anc_out), "%s: win_out and anc_out need windows", fn);
    REQUIRE(n_rec > 0, "%s: no recipients", fn);
    const uint32_t mu = params->mismatch_cost, np = params->n_panels, np1 = np + 1;
    REQUIRE(mu >= 1 && mu <= PAINT_MAX_MU, "%s: mismatch_cost %u is outside 1 .. %u", fn, mu, PAINT_MAX_MU);
    if (n_rec > IMPOP_PAINT_MAX_RECIPIENTS) {
        set_error("%s: %u recipients exceed the limit (%u)", fn, n_rec, (uint32_t)IMPOP_PAINT_MAX_RECIPIENTS);
        return IMPOP_E_UNSUPPORTED;
    }
    if (np > IMPOP_PAINT_MAX_PANELS) {
        set_error("%s: %u panels exceed the limit (%u)", fn, np, (uint32_t)IMPOP_PAINT_MAX_PANELS);
        return IMPOP_E_UNSUPPORTED;
    }
    const uint32_t nh = m->g.n_hap, wps = m->g.wps, n_pad = wps * 32;
    // the range's columns and stored sites
    const uint64_t cb = m->compact ? pos_lower_bound(m, b) : b, ce = m->compact ? pos_lower_bound(m, e) : e;
    REQUIRE(ce > cb, "%s: the range [%llu,%llu) holds no kept site of the compacted matrix", fn, (unsigned long long)b, (unsigned long long)e);
    const uint32_t L = (uint32_t)(ce - cb);
    const uint32_t *csw = params->site_switch_cost;
    if (csw) {
        REQUIRE(params->n_site_switch_cost == L, "%s: site_switch_cost has %llu entries, the range %u stored sites", fn,
                (unsigned long long)params->n_site_switch_cost, L);
        for (uint32_t s = 1; s < L; ++s)
            REQUIRE(csw[s] <= PAINT_MAX_COST, "%s: site_switch_cost[%u] = %u exceeds %u", fn, s, csw[s], PAINT_MAX_COST);
    } else {
        REQUIRE(params->switch_cost <= PAINT_MAX_COST, "%s: switch_cost %u exceeds %u", fn, params->switch_cost, PAINT_MAX_COST);
    }
    REQUIRE(np == 0 || params->panel, "%s: n_panels = %u without a panel array", fn, np);
    std::vector<uint8_t> pslot(nh, (uint8_t)PAINT_NO_PANEL_SLOT);
    for (uint32_t h = 0; params->panel && h < nh; ++h) {
        const uint8_t p = params->panel[h];
        REQUIRE(p < np || p == IMPOP_PAINT_NO_PANEL, "%s: panel[%u] = %u is neither below n_panels = %u nor 255", fn, h, (uint32_t)p, np);
        if (p < np) pslot[h] = p;
    }
    for (uint64_t i = 0; i < (windows ? n_windows : 0); ++i)
        REQUIRE(windows[i].site_begin <= windows[i].site_end, "%s: window %llu [%llu,%llu) ends before it begins", fn, (unsigned long long)i,
                (unsigned long long)windows[i].site_begin, (unsigned long long)windows[i].site_end);

    // recipients, donors, the admissible donors of every recipient
    const MemberSet D = member_set(mask_d, nh, wps);
    std::vector<uint64_t> used((nh + 63) / 64, 0ull);
    for (uint32_t i = 0; i < n_rec; ++i) {
        const uint32_t h = recipients[i];
        REQUIRE(h < nh, "%s: recipient %u: haplotype index %u outside the matrix's %u", fn, i, h, nh);
        REQUIRE(!((used[h >> 6] >> (h & 63)) & 1ull), "%s: recipient %u: haplotype %u is listed twice", fn, i, h);
        used[h >> 6] |= 1ull << (h & 63);
    }
    const uint32_t *grp = params->group;
    std::vector<uint32_t> ndon(n_rec, 0);
    uint32_t max_nd = 0;
    for (uint32_t i = 0; i < n_rec; ++i) {
        const uint32_t h = recipients[i], gi = grp ? grp[h] : h;
        uint32_t k = 0;
        for (uint32_t j : D.idx) k += (grp ? grp[j] : j) != gi ? 1u : 0u;
        REQUIRE(k >= 1, "%s: recipient %u (haplotype %u) has no admissible donor", fn, i, h);
        if (k > IMPOP_PAINT_MAX_DONORS) {
            set_error("%s: recipient %u (haplotype %u) has %u admissible donors, the limit is %u", fn, i, h, k, (uint32_t)IMPOP_PAINT_MAX_DONORS);
            return IMPOP_E_UNSUPPORTED;
        }
        ndon[i] = k;
        max_nd = std::max(max_nd, k);
    }
    // rows: donors and recipients
    for (uint32_t j : D.idx) used[j >> 6] |= 1ull << (j & 63);
    const MemberSet U = member_set(used.data(), nh, wps);
    const uint32_t stride = U.size(), dstride = max_nd;
    std::vector<uint32_t> rrow(n_rec), drow((size_t)n_rec * dstride, 0u);
    for (uint32_t i = 0; i < n_rec; ++i) {
        const uint32_t h = recipients[i], gi = grp ? grp[h] : h;
        rrow[i] = (uint32_t)U.ppos[h];
        uint32_t k = 0;
        for (uint32_t j : D.idx)
            if ((grp ? grp[j] : j) != gi) drow[(size_t)i * dstride + k++] = (uint32_t)U.ppos[j];
    }
    const int Q = max_nd <= 64 ? 1 : max_nd <= 128 ? 2 : max_nd <= 256 ? 4 : max_nd <= 512 ? 8 : 16;

    // windows as stored-site ranges inside the range
    const bool want_win = windows && n_windows > 0 && (win_out || anc_out);
    const uint64_t n_win = want_win ? n_windows : 0;
    REQUIRE(n_win * n_rec < (1ull << 31), "%s: %llu windows x %u recipients exceed one launch", fn, (unsigned long long)n_win, n_rec);
    std::vector<uint32_t> wlo(n_win), whi(n_win);
    for (uint64_t i = 0; i < n_win; ++i) {
        const uint64_t lo = std::min(std::max<uint64_t>(windows[i].site_begin, b), e), hi = std::min(std::max<uint64_t>(windows[i].site_end, b), e);
        wlo[i] = (uint32_t)((m->compact ? pos_lower_bound(m, lo) : lo) - cb);
        whi[i] = (uint32_t)((m->compact ? pos_lower_bound(m, hi) : hi) - cb);
    }

    // the cut: site chunks whose words fit half the budget, recipient ranges whose records fit the other half
    const uint64_t blk0 = cb >> 6, n_blk = ((ce + 63) >> 6) - blk0, budget = chunk_budget(params->max_chunk_bytes);
    const uint32_t env_blocks = env_tile_blocks("IMPOP_PAINT_CHUNK_BLOCKS");
    const uint64_t chunk_blocks = std::min<uint64_t>(n_blk, env_blocks ? env_blocks : std::max<uint64_t>(1, (budget / 2) / ((uint64_t)stride * 8)));
    const uint64_t n_chunks = (n_blk + chunk_blocks - 1) / chunk_blocks;
    const uint32_t range_len = (uint32_t)std::min<uint64_t>(n_rec, std::max<uint64_t>(1, (budget / 2) / ((uint64_t)L * sizeof(PaintRec))));
    const uint32_t n_ranges = (n_rec + range_len - 1) / range_len;

    Carve Lc;
    const size_t o_ppos = Lc.take<int32_t>(n_pad), o_pmask = Lc.take<uint32_t>(wps), o_rows = Lc.take<uint32_t>(stride),
                 o_rrow = Lc.take<uint32_t>(n_rec), o_rhap = Lc.take<uint32_t>(n_rec), o_ndon = Lc.take<uint32_t>(n_rec),
                 o_drow = Lc.take<uint32_t>(drow.size()), o_pslot = Lc.take<uint8_t>(nh), o_csw = Lc.take<uint32_t>(csw ? L : 0),
                 o_wlo = Lc.take<uint32_t>(n_win), o_whi = Lc.take<uint32_t>(n_win), o_cost = Lc.take<unsigned long long>(n_rec),
                 o_nseg = Lc.take<uint32_t>(n_rec), o_out = Lc.take<impop_paint_recipient>(n_rec), o_win = Lc.take<impop_paint_window>(n_win),
                 o_anc = Lc.take<uint32_t>(anc_out ? n_win * n_rec * np1 : 0), o_wm = Lc.take<uint64_t>(chunk_blocks * stride),
                 o_rec = Lc.take<PaintRec>((uint64_t)range_len * L), o_stR = Lc.take<uint32_t>((uint64_t)range_len * Q * 64),
                 o_stT = Lc.take<uint32_t>((uint64_t)range_len * Q * 64), o_off = Lc.take<uint64_t>(range_len + 1),
                 o_cc = Lc.take<uint32_t>((uint64_t)range_len * nh), o_cs = Lc.take<unsigned long long>((uint64_t)range_len * nh);
    HIP_TRY(hipSetDevice(ctx->device));
    void *d = nullptr;
    int rc = ctx_scratch(ctx, Lc.total(), &d);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    const std::vector<uint32_t> rhap(recipients, recipients + n_rec);
    auto up = [&](size_t off, const void *src, size_t bytes) -> int {
        if (bytes) HIP_TRY(hipMemcpyAsync(Lc.at<char>(d, off), src, bytes, hipMemcpyHostToDevice, st));
        return IMPOP_OK;
    };
    if ((rc = up(o_ppos, U.ppos.data(), (size_t)n_pad * 4)) || (rc = up(o_pmask, U.bits.data(), (size_t)wps * 4)) ||
        (rc = up(o_rows, U.idx.data(), (size_t)stride * 4)) || (rc = up(o_rrow, rrow.data(), (size_t)n_rec * 4)) ||
        (rc = up(o_rhap, rhap.data(), (size_t)n_rec * 4)) || (rc = up(o_ndon, ndon.data(), (size_t)n_rec * 4)) ||
        (rc = up(o_drow, drow.data(), drow.size() * 4)) || (rc = up(o_pslot, pslot.data(), nh)) ||
        (rc = up(o_csw, csw, csw ? (size_t)L * 4 : 0)) || (rc = up(o_wlo, wlo.data(), n_win * 4)) || (rc = up(o_whi, whi.data(), n_win * 4)))
        return rc;
    if (n_win) HIP_TRY(hipMemsetAsync(Lc.at<char>(d, o_win), 0, n_win * sizeof(impop_paint_window), st));
    if (anc_out && n_win) HIP_TRY(hipMemsetAsync(Lc.at<char>(d, o_anc), 0, n_win * n_rec * np1 * 4, st));

    PaintArgs A{};
    A.wm = Lc.at<uint64_t>(d, o_wm);
    A.pos = m->compact ? m->d_pos : nullptr;
    A.csw = csw ? Lc.at<uint32_t>(d, o_csw) : nullptr;
    A.ppos = Lc.at<int32_t>(d, o_ppos);
    A.rows = Lc.at<uint32_t>(d, o_rows);
    A.rrow = Lc.at<uint32_t>(d, o_rrow);
    A.rhap = Lc.at<uint32_t>(d, o_rhap);
    A.ndon = Lc.at<uint32_t>(d, o_ndon);
    A.drow = Lc.at<uint32_t>(d, o_drow);
    A.pslot = Lc.at<uint8_t>(d, o_pslot);
    A.rec = Lc.at<PaintRec>(d, o_rec);
    A.stR = Lc.at<uint32_t>(d, o_stR);
    A.stT = Lc.at<uint32_t>(d, o_stT);
    A.cost = Lc.at<unsigned long long>(d, o_cost);
    A.nseg = Lc.at<uint32_t>(d, o_nseg);
    A.off = Lc.at<uint64_t>(d, o_off);
    A.cc = Lc.at<uint32_t>(d, o_cc);
    A.cs = Lc.at<unsigned long long>(d, o_cs);
    A.out = Lc.at<impop_paint_recipient>(d, o_out);
    A.win = Lc.at<impop_paint_window>(d, o_win);
    A.wlo = Lc.at<uint32_t>(d, o_wlo);
    A.whi = Lc.at<uint32_t>(d, o_whi);
    A.anc = anc_out && n_win ? Lc.at<uint32_t>(d, o_anc) : nullptr;
    A.err = ctx->d_err;
    A.b = b;
    A.e = e;
    A.cb = cb;
    A.L = L;
    A.stride = stride;
    A.dstride = dstride;
    A.n_rec = n_rec;
    A.n_hap = nh;
    A.mu = mu;
    A.cconst = params->switch_cost;
    A.np1 = np1;
    A.n_win = (uint32_t)n_win;

    EventPairs *timer = ctx->timers + (int)impop_ctx::T_PAINT;
    uint64_t launches = 0, bytes_streamed = 0, chunks_run = 0, total = 0;
    auto transpose = [&](uint64_t c) -> int {
        A.blk_abs0 = blk0 + c * chunk_blocks;
        A.len = std::min<uint64_t>(chunk_blocks, n_blk - c * chunk_blocks);
        ++launches;
        ++chunks_run;
        bytes_streamed += A.len * 64 * wps * 4;
        return timed(ctx, timer[0], [&] {
            hipLaunchKernelGGL(ibs_transpose_kernel, dim3((uint32_t)((A.len + 3) / 4)), dim3(256), 0, st, m->d_sb, wps, m->g.G, m->g.r,
                               Lc.at<int32_t>(d, o_ppos), Lc.at<uint32_t>(d, o_pmask), A.blk_abs0, A.len, cb, ce, stride,
                               Lc.at<uint64_t>(d, o_wm));
        });
    };
    auto sync_checked = [&]() -> int {
        const int rc2 = ctx_err_fetch(ctx);
        if (rc2) return rc2;
        HIP_TRY(hipStreamSynchronize(st));
        return ctx_err_result(ctx, fn);
    };
    if (n_chunks == 1 && (rc = transpose(0))) return rc;  // the words serve every recipient range

    const bool keep_seg = seg_out && seg_capacity > 0;
    std::vector<impop_paint_segment> hseg;  // the list is handed over only once the total is known to fit
    bool seg_fits = keep_seg;
    std::vector<uint32_t> h_nseg(range_len);
    std::vector<uint64_t> h_off(range_len + 1);
    for (uint32_t g = 0; g < n_ranges; ++g) {
        A.r0 = g * range_len;
        A.r1 = std::min<uint32_t>(n_rec, A.r0 + range_len);
        const uint32_t nr = A.r1 - A.r0;
        uint64_t words_per_block = 0;
        for (uint32_t r = A.r0; r < A.r1; ++r) words_per_block += ndon[r] + 1;
        for (uint64_t c = 0; c < n_chunks; ++c) {
            if (n_chunks > 1 && (rc = transpose(c))) return rc;
            const int first = c == 0;
            if ((rc = timed(ctx, timer[1], [&] {
                    switch (Q) {
                    case 1: paint_launch_forward<1>(ctx, A, first); break;
                    case 2: paint_launch_forward<2>(ctx, A, first); break;
                    case 4: paint_launch_forward<4>(ctx, A, first); break;
                    case 8: paint_launch_forward<8>(ctx, A, first); break;
                    default: paint_launch_forward<16>(ctx, A, first); break;
                    }
                })))
                return rc;
            ++launches;
            bytes_streamed += A.len * words_per_block * 8;
        }
        // count -> offsets
        if ((rc = timed(ctx, timer[2], [&] { hipLaunchKernelGGL(paint_backtrack_kernel, dim3((nr + 63) / 64), dim3(64), 0, st, A, 0); }))) return rc;
        ++launches;
        HIP_TRY(hipMemcpyAsync(h_nseg.data(), A.nseg + A.r0, (size_t)nr * 4, hipMemcpyDeviceToHost, st));
        if ((rc = sync_checked())) return rc;
        h_off[0] = 0;
        for (uint32_t i = 0; i < nr; ++i) h_off[i + 1] = h_off[i] + h_nseg[i];
        const uint64_t cnt = h_off[nr];
        Carve L2;
        const size_t o_seg = L2.take<impop_paint_segment>(cnt), o_s0 = L2.take<uint32_t>(cnt);
        void *d2 = nullptr;
        if ((rc = ctx_aux(ctx, 0, L2.total() + 256, &d2))) return rc;
        A.seg = L2.at<impop_paint_segment>(d2, o_seg);
        A.seg_s0 = L2.at<uint32_t>(d2, o_s0);
        HIP_TRY(hipMemcpyAsync(Lc.at<char>(d, o_off), h_off.data(), (size_t)(nr + 1) * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(A.cc, 0, (size_t)nr * nh * 4, st));
        HIP_TRY(hipMemsetAsync(A.cs, 0, (size_t)nr * nh * 8, st));
        if ((rc = timed(ctx, timer[2], [&] { hipLaunchKernelGGL(paint_backtrack_kernel, dim3((nr + 63) / 64), dim3(64), 0, st, A, 1); }))) return rc;
        ++launches;
        // the words once more: mismatches of the segments and of the windows
        for (uint64_t c = 0; c < n_chunks; ++c) {
            if (n_chunks > 1 && (rc = transpose(c))) return rc;
            if (n_chunks == 1) {
                A.blk_abs0 = blk0;
                A.len = n_blk;
            }
            if ((rc = timed(ctx, timer[2], [&] {
                    hipLaunchKernelGGL(paint_mismatch_kernel, dim3((uint32_t)((cnt + 3) / 4)), dim3(256), 0, st, A, cnt);
                })))
                return rc;
            ++launches;
            if (n_win) {
                if ((rc = timed(ctx, timer[3], [&] {
                        hipLaunchKernelGGL(paint_window_kernel, dim3((uint32_t)(n_win * nr)), dim3(64), 0, st, A, c == 0 ? 1 : 0);
                    })))
                    return rc;
                ++launches;
            }
        }
        if ((rc = timed(ctx, timer[2], [&] { hipLaunchKernelGGL(paint_record_kernel, dim3(nr), dim3(64), 0, st, A); }))) return rc;
        ++launches;
        if (chunk_counts) HIP_TRY(hipMemcpyAsync(chunk_counts + (size_t)A.r0 * nh, A.cc, (size_t)nr * nh * 4, hipMemcpyDeviceToHost, st));
        if (chunk_sites) HIP_TRY(hipMemcpyAsync(chunk_sites + (size_t)A.r0 * nh, A.cs, (size_t)nr * nh * 8, hipMemcpyDeviceToHost, st));
        if (seg_fits && total + cnt <= seg_capacity) {
            hseg.resize(total + cnt);
            HIP_TRY(hipMemcpyAsync(hseg.data() + total, A.seg, cnt * sizeof(impop_paint_segment), hipMemcpyDeviceToHost, st));
        } else {
            seg_fits = false;
        }
        total += cnt;
        if ((rc = sync_checked())) return rc;
    }
    if (rec_out) HIP_TRY(hipMemcpyAsync(rec_out, A.out, (size_t)n_rec * sizeof(impop_paint_recipient), hipMemcpyDeviceToHost, st));
    if (win_out && n_win) HIP_TRY(hipMemcpyAsync(win_out, A.win, n_win * sizeof(impop_paint_window), hipMemcpyDeviceToHost, st));
    if (anc_out && n_win) HIP_TRY(hipMemcpyAsync(anc_out, A.anc, n_win * n_rec * np1 * 4, hipMemcpyDeviceToHost, st));
    if ((rc = sync_checked())) return rc;
    *n_segments = total;
    if (seg_fits && total) memcpy(seg_out, hseg.data(), total * sizeof(impop_paint_segment));
    if (trace_on()) {
        fprintf(stderr,
                "[impop_paint_scan] route=%s recipients=%u donors=%u sites=%u site_chunks=%llu recipient_ranges=%u segments=%llu launches=%llu "
                "bytes_streamed=%llu\n",
                m->compact ? "compact" : "dense", n_rec, D.size(), L, (unsigned long long)chunks_run, n_ranges, (unsigned long long)total,
                (unsigned long long)launches, (unsigned long long)bytes_streamed);
        fflush(stderr);
    }
    return IMPOP_OK;
}

IMPOP_API int impop_ctx_paint_elapsed(impop_ctx *ctx, double kernel_ms[4], uint64_t *chunks) {
    REQUIRE(ctx && kernel_ms, "impop_ctx_paint_elapsed: NULL argument");
    return ctx_timers_elapsed(ctx, impop_ctx::T_PAINT, 4, 1, kernel_ms, chunks);
}
