// ibd.hip — impop_ibd_scan: IBD segments from a pair's exact IBS tracts, gaps and a genetic map (include/impop_hip.h).
//
// Two stages per pair range of the segment staging (ibs_sweeps.h):
//   1. the count and fill sweeps of ibs.hip with min_sites leave the range's tracts of extent >= min_sites on the device,
//      pair-major and ascending;
//   2. ibd_chain_kernel, the WAVE form: one wave per pair, the lanes take 64 consecutive staged tracts.  A lane evaluates G at
//      both ends of its tract (binary search over the breakpoints, staged in LDS when they fit, else read from global memory),
//      its class and whether it opens a chain; ballots of these give the chains as bit ranges (ibd_chain.h), a prefix sum over the
//      lanes their sums; the chain left open is carried from batch to batch in wave-uniform state.
//      count form: the pair record.  Host: prefix over n_segments of the range.  fill form: every segment at the pair's offset,
//      added to the window tables (ibs_plan.h) with integer atomics.
// The segments of a range are copied to the host and buffered there until the total is known (they are far fewer than the
// candidates).  A segment at or past the pair's announced count is never written: it sets DEV_ERR_IBD.  Every loop is bounded by
// a count from the host or from the count form; no spin waits, no flags between workgroups.
#include <string.h>

#include <algorithm>
#include <vector>

#include "chunk_run.h"
#include "ibd_chain.h"
#include "ibs_plan.h"
#include "ibs_sweeps.h"
#include "internal.h"

namespace impop {

constexpr int IBD_T = 256;               // four waves = four pairs in flight per workgroup
constexpr uint32_t IBD_MAP_LDS = 2048;   // breakpoints staged in LDS (32 KiB); a longer map is read from global memory

struct IbdArgs {
    const impop_ibs_segment *seg;  // the staged tracts
    const uint64_t *off;           // all pairs' tract offsets
    const impop_ibs_pair *rec;     // h1, h2
    impop_ibd_pair *prec;          // count: the records of [p0, p1), entry pair - p0
    const uint64_t *soff;          // fill: the segment offsets of [p0, p1) inside the range, p1 - p0 + 1 entries
    impop_ibd_segment *sout;       // fill: the range's segments
    uint32_t *err;
    IbsWindowsDev win;             // acc null: no windows
    IbdMap map;
    IbdRule rule;
    uint64_t off0, p0, p1, b, e;
};

__device__ inline uint64_t shfl64(uint64_t v, uint32_t src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, (int)src, 64), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), (int)src, 64);
    return ((uint64_t)hi << 32) | lo;
}
__device__ inline uint64_t uniform64(uint64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}
__device__ inline uint64_t wave_sum64(uint64_t v) {
    for (int o = 32; o > 0; o >>= 1) v += shfl64(v, (threadIdx.x & 63) ^ o);
    return v;
}
__device__ inline uint64_t wave_max64(uint64_t v) {
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t w = shfl64(v, (threadIdx.x & 63) ^ o);
        v = w > v ? w : v;
    }
    return v;
}

struct IbdLaneSums {  // what a lane's reported chains add to the pair record
    uint64_t len = 0, extent = 0, longest = 0, sites = 0;
};

// the reported chain c is segment k of `pair`
template <bool FILL>
__device__ inline void ibd_emit(const IbdArgs &A, IbdLaneSums &acc, const IbdChain &c, uint64_t pair, uint32_t h1, uint32_t h2, uint32_t k,
                                uint32_t announced, uint64_t sbase) {
    const uint64_t len = c.gend - c.gbegin;
    if (!FILL) {
        acc.len += len;
        acc.extent += c.end - c.begin;
        acc.sites += c.sites;
        acc.longest = len > acc.longest ? len : acc.longest;
        return;
    }
    if (k >= announced) {  // the count form did not announce it: nothing is written
        atomicOr(A.err, DEV_ERR_IBD);
        return;
    }
    impop_ibd_segment o;
    o.h1 = h1;
    o.h2 = h2;
    o.begin = c.begin;
    o.end = c.end;
    o.len = len;
    o.ibs_sites = c.sites;
    o.n_tracts = c.n;
    o.pair = (uint32_t)pair;
    o.flags = (c.begin == A.b ? IMPOP_IBS_OPEN_LEFT : 0u) | (c.end == A.e ? IMPOP_IBS_OPEN_RIGHT : 0u);
    A.sout[sbase + k] = o;
    if (A.win.acc) ibs_add_tract(A.win, c.begin, c.end, [](unsigned long long *p, unsigned long long v) { atomicAdd(p, v); });
}

// grid = min(ceil(pairs / 4), a few workgroups per compute unit): a wave takes the pairs p0 + its index, + the grid's waves, ...
template <bool FILL>
__global__ __launch_bounds__(IBD_T) void ibd_chain_kernel(const IbdArgs A) {
    __shared__ uint64_t s_map[2 * IBD_MAP_LDS];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    IbdMap map = A.map;
    if (map.n != 0 && map.n <= IBD_MAP_LDS) {
        for (uint32_t i = tid; i < map.n; i += IBD_T) {
            s_map[i] = A.map.pos[i];
            s_map[IBD_MAP_LDS + i] = A.map.g[i];
        }
        map.pos = s_map;
        map.g = s_map + IBD_MAP_LDS;
    }
    __syncthreads();  // the only barrier: every wave passes it once, before its pairs
    const IbdRule rule = A.rule;
    const uint64_t step = (uint64_t)gridDim.x * (IBD_T / 64);
    for (uint64_t pair = A.p0 + (uint64_t)blockIdx.x * (IBD_T / 64) + wave; pair < A.p1; pair += step) {  // wave-uniform
        const uint64_t t0 = uniform64(A.off[pair] - A.off0), t1 = uniform64(A.off[pair + 1] - A.off0);
        const impop_ibs_pair pr = A.rec[pair];
        uint64_t sbase = 0;
        uint32_t announced = 0;
        if (FILL) {
            sbase = uniform64(A.soff[pair - A.p0]);
            announced = (uint32_t)(uniform64(A.soff[pair - A.p0 + 1]) - sbase);
        }
        IbdChain c;            // the open chain: the same in every lane
        IbdLaneSums acc;       // this lane's share of the pair record
        uint32_t k = 0, n_cand = 0;  // uniform: chains reported, candidates seen
        for (uint64_t base = t0; base < t1; base += 64) {
            const bool on = base + lane < t1;
            uint64_t s = 0, t = 0;
            if (on) {
                const impop_ibs_segment g = A.seg[base + lane];
                s = g.begin;
                t = g.end;
            }
            const uint64_t gs = on ? ibd_map_eval(map, s) : 0, gt = on ? ibd_map_eval(map, t) : 0;
            const uint32_t cls = on ? ibd_class(rule, t - s, gt - gs) : 0u;
            const bool cand = (cls & IBD_CANDIDATE) != 0;
            const uint64_t cmask = __ballot(cand), smask = __ballot((cls & IBD_SEED) != 0);
            const uint32_t ext = cand ? (uint32_t)(t - s) : 0u;
            uint32_t pre = ext;  // inclusive prefix over the lanes
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t v = (uint32_t)__shfl_up((int)pre, d, 64);
                if ((int)lane >= d) pre += v;
            }
            const int pl = ibd_prev_lane(cmask, lane);
            const uint64_t pt = shfl64(t, pl >= 0 ? (uint32_t)pl : lane);
            const bool brk = cand && ibd_breaks(pl >= 0 || c.open, pl >= 0 ? pt : c.end, s, rule.max_gap);
            const uint64_t bmask = __ballot(brk);
            n_cand += (uint32_t)__builtin_popcountll(cmask);
            const uint64_t head = ibd_head_lanes(cmask, bmask);
            if (head) {  // uniform
                const uint32_t top = ibd_top_lane(head);
                ibd_chain_extend(c, shfl64(t, top), shfl64(gt, top), (uint32_t)__builtin_popcountll(head), (uint32_t)__shfl((int)pre, (int)top, 64),
                                 (smask & head) != 0);
            }
            if (!bmask) continue;  // uniform
            if (ibd_reported(c, rule)) {
                if (lane == 0) ibd_emit<FILL>(A, acc, c, pair, pr.h1, pr.h2, k, announced, sbase);
                ++k;
            }
            // every head builds its chain; all but the last one's close inside the batch
            const uint32_t last = ibd_top_lane(bmask);
            const uint64_t lanes = brk ? ibd_chain_lanes(cmask, bmask, lane) : (1ull << lane);
            const uint32_t top = ibd_top_lane(lanes);
            const uint64_t te = shfl64(t, top), gte = shfl64(gt, top);
            const uint32_t ptop = (uint32_t)__shfl((int)pre, (int)top, 64);
            const IbdChain mine = ibd_chain_make(s, gs, te, gte, (uint32_t)__builtin_popcountll(lanes), ptop - pre + ext, (smask & lanes) != 0);
            const bool rep = brk && lane != last && ibd_reported(mine, rule);
            const uint64_t rmask = __ballot(rep);
            if (rep) ibd_emit<FILL>(A, acc, mine, pair, pr.h1, pr.h2, k + (uint32_t)__builtin_popcountll(rmask & ibd_lanes_below(lane)), announced, sbase);
            k += (uint32_t)__builtin_popcountll(rmask);
            c = ibd_chain_make(shfl64(s, last), shfl64(gs, last), shfl64(te, last), shfl64(gte, last), (uint32_t)__shfl((int)mine.n, (int)last, 64),
                               (uint32_t)__shfl((int)mine.sites, (int)last, 64), __shfl((int)mine.seed, (int)last, 64) != 0);
        }
        if (ibd_reported(c, rule)) {
            if (lane == 0) ibd_emit<FILL>(A, acc, c, pair, pr.h1, pr.h2, k, announced, sbase);
            ++k;
        }
        if (FILL) {
            if (lane == 0 && k != announced) atomicOr(A.err, DEV_ERR_IBD);
        } else {
            impop_ibd_pair o;
            o.h1 = pr.h1;
            o.h2 = pr.h2;
            o.n_segments = k;
            o.n_candidates = n_cand;
            o.total_len = wave_sum64(acc.len);
            o.total_extent = wave_sum64(acc.extent);
            o.longest_len = wave_max64(acc.longest);
            o.ibs_sites = wave_sum64(acc.sites);
            if (lane == 0) A.prec[pair - A.p0] = o;
        }
    }
}

}  // namespace impop

using namespace impop;

IMPOP_API int impop_ibd_scan(impop_ctx *ctx, const impop_matrix *m, const uint64_t *mask_p, const uint32_t *pairs, uint64_t n_pairs,
                             const impop_window *windows, uint64_t n_windows, const impop_ibd_params *params, impop_ibd_pair *pair_out,
                             impop_ibd_segment *seg_out, uint64_t seg_capacity, uint64_t *n_segments, impop_ibs_window *win_out) {
    static_assert(sizeof(impop_ibd_params) == 88 && sizeof(impop_ibd_pair) == 48 && sizeof(impop_ibd_segment) == 48, "ABI layout");
    const char *fn = "impop_ibd_scan";
    REQUIRE(ctx && m && params && n_segments, "%s: NULL argument", fn);
    REQUIRE(params->struct_size == sizeof(impop_ibd_params), "impop_ibd_params.struct_size mismatch");
    REQUIRE(params->min_seed >= params->min_extend, "%s: min_seed (%llu) is below min_extend (%llu)", fn,
            (unsigned long long)params->min_seed, (unsigned long long)params->min_extend);
    const uint64_t n_map = params->n_map;
    REQUIRE((params->map_pos == nullptr) == (params->map_g == nullptr) && (params->map_pos != nullptr) == (n_map != 0),
            "%s: map_pos and map_g must both hold n_map breakpoints, or both be NULL with n_map 0", fn);
    REQUIRE(n_map != 1, "%s: a map of one breakpoint has no rate", fn);
    if (n_map > IMPOP_IBD_MAX_MAP) {
        set_error("%s: %llu map breakpoints exceed the limit (%u)", fn, (unsigned long long)n_map, (uint32_t)IMPOP_IBD_MAX_MAP);
        return IMPOP_E_UNSUPPORTED;
    }
    if (n_map) {
        const uint64_t bad = ibd_map_check(params->map_pos, params->map_g, n_map);
        REQUIRE(bad == 0, "%s: map breakpoint %llu: pos must ascend strictly, g must not decrease, and both steps must be below 2^32", fn,
                (unsigned long long)bad);
    }
    REQUIRE((windows == nullptr) == (win_out == nullptr), "%s: windows and win_out must both be given or both be NULL", fn);
    const uint64_t b = params->site_begin, e = params->site_end ? params->site_end : matrix_span(m);
    for (uint64_t i = 0; i < (windows ? n_windows : 0); ++i)
        REQUIRE(b <= windows[i].site_begin && windows[i].site_begin <= windows[i].site_end && windows[i].site_end <= e,
                "%s: window %llu [%llu,%llu) is not inside the range [%llu,%llu)", fn, (unsigned long long)i,
                (unsigned long long)windows[i].site_begin, (unsigned long long)windows[i].site_end, (unsigned long long)b,
                (unsigned long long)e);
    const bool want_win = windows && n_windows > 0;

    // the breakpoints that bracket the range: G over [b, e] does not change when the others are left out
    uint64_t k0 = 0, k1 = n_map;
    if (n_map) {
        k0 = (uint64_t)(std::upper_bound(params->map_pos, params->map_pos + n_map, b) - params->map_pos);
        k0 = k0 ? k0 - 1 : 0;  // the last breakpoint at or left of b
        k1 = (uint64_t)(std::lower_bound(params->map_pos, params->map_pos + n_map, e) - params->map_pos);
        k1 = std::min(n_map, k1 + 1);  // the first at or right of e, included
        if (k1 - k0 < 2) {  // the range lies outside the map: G is constant there; keep two points so the map stays a map
            if (k0 > 0) --k0;
            else k1 = 2;
        }
    }
    const uint32_t n_up = (uint32_t)(k1 - k0);

    IbsWindowPlan wp;
    if (want_win) {
        std::vector<uint64_t> wb(n_windows), we(n_windows);
        for (uint64_t i = 0; i < n_windows; ++i) {
            wb[i] = windows[i].site_begin;
            we[i] = windows[i].site_end;
        }
        wp.build(wb.data(), we.data(), n_windows);
    }

    // the call's own device memory: map | window tables | their sums
    Carve L;
    const size_t o_mpos = L.take<uint64_t>(n_up), o_mg = L.take<uint64_t>(n_up), o_edge = L.take<uint64_t>(wp.edge.size()),
                 o_sbeg = L.take<uint64_t>(wp.sbeg.size()), o_send = L.take<uint64_t>(wp.send.size()),
                 o_acc = L.take<unsigned long long>(want_win ? wp.acc_words() : 0);
    hipStream_t st = ctx->stream;
    IbdArgs A{};
    A.err = ctx->d_err;
    A.rule.min_seed = params->min_seed;
    A.rule.min_extend = params->min_extend;
    A.rule.min_output = params->min_output;
    A.rule.max_gap = params->max_gap;
    A.rule.min_sites = params->min_sites;
    A.b = b;
    A.e = e;
    const bool want_fill = seg_out != nullptr || want_win;
    std::vector<impop_ibd_pair> rec_host;
    std::vector<impop_ibd_segment> seg_host;  // the segments of the ranges so far
    std::vector<uint64_t> soff;
    uint64_t total = 0, candidates = 0, launches = 0;
    char *d_own = nullptr;

    IbsClient client;
    client.timer = impop_ctx::T_IBD;
    client.extra_bytes = L.total();
    client.prepare = [&](void *d_extra, uint64_t np) -> int {
        d_own = static_cast<char *>(d_extra);
        if (n_up) {
            HIP_TRY(hipMemcpyAsync(d_own + o_mpos, params->map_pos + k0, (size_t)n_up * 8, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(d_own + o_mg, params->map_g + k0, (size_t)n_up * 8, hipMemcpyHostToDevice, st));
            A.map.pos = L.at<uint64_t>(d_own, o_mpos);
            A.map.g = L.at<uint64_t>(d_own, o_mg);
            A.map.n = n_up;
        }
        if (want_win) {
            HIP_TRY(hipMemcpyAsync(d_own + o_edge, wp.edge.data(), wp.edge.size() * 8, hipMemcpyHostToDevice, st));
            if (!wp.sbeg.empty()) {
                HIP_TRY(hipMemcpyAsync(d_own + o_sbeg, wp.sbeg.data(), wp.sbeg.size() * 8, hipMemcpyHostToDevice, st));
                HIP_TRY(hipMemcpyAsync(d_own + o_send, wp.send.data(), wp.send.size() * 8, hipMemcpyHostToDevice, st));
            }
            HIP_TRY(hipMemsetAsync(d_own + o_acc, 0, wp.acc_words() * 8, st));
            A.win.edge = L.at<uint64_t>(d_own, o_edge);
            A.win.sbeg = L.at<uint64_t>(d_own, o_sbeg);
            A.win.send = L.at<uint64_t>(d_own, o_send);
            A.win.acc = L.at<unsigned long long>(d_own, o_acc);
            A.win.n_edge = (uint32_t)wp.edge.size();
            A.win.n_span = (uint32_t)wp.sbeg.size();
        }
        if (!pair_out) rec_host.resize(np);
        return IMPOP_OK;
    };
    auto sync_checked = [&]() -> int {
        const int rc2 = ctx_err_fetch(ctx);
        if (rc2) return rc2;
        HIP_TRY(hipStreamSynchronize(st));
        return ctx_err_result(ctx, fn);
    };
    client.range = [&](const IbsStage &S) -> int {
        int rc2;
        const uint64_t np = S.p1 - S.p0;
        impop_ibd_pair *recs = (pair_out ? pair_out : rec_host.data()) + S.p0;
        const uint32_t grid = (uint32_t)std::min<uint64_t>((np + IBD_T / 64 - 1) / (IBD_T / 64), 16ull * (ctx->n_cu > 0 ? ctx->n_cu : 1));
        // count: the pair records.  Side buffer 1: records, then (their contents are on the host by then) offsets | segments
        void *d1 = nullptr;
        if ((rc2 = ctx_aux(ctx, 1, np * sizeof(impop_ibd_pair) + 256, &d1))) return rc2;
        A.seg = S.d_seg;
        A.off = S.d_off;
        A.rec = S.d_rec;
        A.off0 = S.off0;
        A.p0 = S.p0;
        A.p1 = S.p1;
        A.prec = static_cast<impop_ibd_pair *>(d1);
        A.soff = nullptr;
        A.sout = nullptr;
        if ((rc2 = timed(ctx, ctx->timers[impop_ctx::T_IBD + 3],
                         [&] { hipLaunchKernelGGL(ibd_chain_kernel<false>, dim3(grid), dim3(IBD_T), 0, st, A); })))
            return rc2;
        ++launches;
        HIP_TRY(hipMemcpyAsync(recs, d1, np * sizeof(impop_ibd_pair), hipMemcpyDeviceToHost, st));
        if ((rc2 = sync_checked())) return rc2;
        soff.assign(np + 1, 0);
        for (uint64_t p = 0; p < np; ++p) {
            soff[p + 1] = soff[p] + recs[p].n_segments;
            candidates += recs[p].n_candidates;
        }
        const uint64_t here = soff[np];
        total += here;
        if (!want_fill || here == 0) return IMPOP_OK;
        // fill: the range's segments and their share of the window tables
        Carve L1;
        const size_t o_soff = L1.take<uint64_t>(np + 1), o_sout = L1.take<impop_ibd_segment>(here);
        if ((rc2 = ctx_aux(ctx, 1, L1.total(), &d1))) return rc2;
        HIP_TRY(hipMemcpyAsync(L1.at<char>(d1, o_soff), soff.data(), (np + 1) * 8, hipMemcpyHostToDevice, st));
        A.prec = nullptr;
        A.soff = L1.at<uint64_t>(d1, o_soff);
        A.sout = L1.at<impop_ibd_segment>(d1, o_sout);
        if ((rc2 = timed(ctx, ctx->timers[impop_ctx::T_IBD + 3],
                         [&] { hipLaunchKernelGGL(ibd_chain_kernel<true>, dim3(grid), dim3(IBD_T), 0, st, A); })))
            return rc2;
        ++launches;
        const size_t at = seg_host.size();
        if (seg_out) {
            seg_host.resize(at + here);
            HIP_TRY(hipMemcpyAsync(seg_host.data() + at, A.sout, here * sizeof(impop_ibd_segment), hipMemcpyDeviceToHost, st));
        }
        return sync_checked();
    };

    uint64_t n_tracts = 0;
    int rc = ibs_scan_run(fn, ctx, m, mask_p, pairs, n_pairs, nullptr, 0, params->site_begin, params->site_end, params->min_sites,
                          params->max_chunk_bytes, nullptr, nullptr, 0, &n_tracts, nullptr, &client);
    if (rc) return rc;
    *n_segments = total;
    if (seg_out && seg_capacity >= total && total > 0) memcpy(seg_out, seg_host.data(), total * sizeof(impop_ibd_segment));
    if (want_win) {
        std::vector<unsigned long long> acc(wp.acc_words(), 0ull);
        if (total > 0) {
            HIP_TRY(hipMemcpyAsync(acc.data(), d_own + o_acc, acc.size() * 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        const std::vector<IbsWindowSums> sums = wp.finish(acc.data());
        for (uint64_t i = 0; i < n_windows; ++i) {
            const uint64_t wb = windows[i].site_begin, we = windows[i].site_end;
            impop_ibs_window o;
            o.pair_sites = sums[i].pair_sites;
            o.tracts = (uint32_t)sums[i].tracts;
            o.pairs_spanning = (uint32_t)sums[i].spanning;
            o.n_sites = (uint32_t)window_W(m, wb, we);
            o.reserved = 0;
            o.share = we > wb ? (double)o.pair_sites / ((double)client.n_pairs * (double)(we - wb)) : __builtin_nan("");
            win_out[i] = o;
        }
    }
    if (trace_on()) {
        fprintf(stderr,
                "[impop_ibd_scan] route=%s pairs=%llu pair_ranges=%llu candidates=%llu segments=%llu map_points=%u launches=%llu "
                "bytes_streamed=%llu\n",
                m->compact ? "compact" : "dense", (unsigned long long)client.n_pairs, (unsigned long long)client.pair_ranges,
                (unsigned long long)candidates, (unsigned long long)total, n_up, (unsigned long long)(client.launches + launches),
                (unsigned long long)(client.bytes_streamed + n_tracts * sizeof(impop_ibs_segment) * (want_fill ? 2 : 1)));
        fflush(stderr);
    }
    return IMPOP_OK;
}

IMPOP_API int impop_ctx_ibd_elapsed(impop_ctx *ctx, double kernel_ms[4], uint64_t *chunks) {
    REQUIRE(ctx && kernel_ms, "impop_ctx_ibd_elapsed: NULL argument");
    return ctx_timers_elapsed(ctx, impop_ctx::T_IBD, 4, 0, kernel_ms, chunks);
}
