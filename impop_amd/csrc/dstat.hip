// dstat.hip — impop_dstat_scan: Patterson's D (ABBA-BABA), f4 and Martin's f_d per window and quartet of populations
// (include/impop_hip.h).  One streaming pass over what scan_route picks — the variable-site index with its rare entries, the
// rows of a weighted matrix, the kept sites of a compacted one.  The pass itself is pop_stream.h, shared with scan_multi_kernel
// (scan.hip): masks of all K populations in LDS, a lane per site, several granules in flight, per-tile integer partials; here a
// finalize kernel adds each window's tile range.  The host half (masks, upload, launch) is shared as well: scan_route.h.
// Every term is zero where the site is monomorphic among all haplotypes, so the sites the index and a
// compaction drop add nothing, with or without polarisation (an outgroup count of 0 or nO is never a tie).
//
// New is the per-site work: from the K counts of a site, per quartet five 64-bit sums and two counters.  The four populations of
// a quartet are disjoint and n <= 65535, so every product of two counts / sizes of different populations is below 2^30: each
// term is ONE 32 x 32 -> 64 multiply-add of two such products (v_mad_u64_u32 / v_mad_i64_i32), plus the weight multiply on
// weighted matrices only.  The accumulators cost 12 VGPRs per quartet, so the quartet list is handled IMPOP_DSTAT_GROUP at a
// time: the same tiles for every group, one streaming and one finalize launch per group (DESIGN.md has the register report the
// group size was chosen from).  The doubles of a record are computed on the host from its integers, in one place.
#include <string.h>

#include <algorithm>
#include <vector>

#include "device_utils.h"
#include "internal.h"
#include "pop_stream.h"
#include "scan_route.h"

namespace impop {

constexpr int DSTAT_QG = (int)IMPOP_DSTAT_GROUP;  // quartets per launch
constexpr int DSTAT_NV = 7;                       // per quartet and tile: abba, baba, f4_num, fd_den_p2, fd_den_p3, n_informative, n_skipped

struct DstatQuartet {  // P1, P2, P3, O
    uint32_t p[4];     // indices into the K populations
    uint32_t n[4];     // their sizes
};
struct DstatGroup {  // a kernel argument: wave-uniform (SGPR) state
    DstatQuartet q[DSTAT_QG];
};

struct DstatAcc {
    uint64_t abba = 0, baba = 0;
    int64_t f4 = 0, fd2 = 0, fd3 = 0;
    uint32_t inf = 0, skip = 0;
};

// One site of one quartet.  All products below are of counts / sizes of two different populations of the quartet: < 2^30.
template <bool WEIGHTED>
__device__ __forceinline__ void dstat_site(uint32_t c1, uint32_t c2, uint32_t c3, uint32_t cO, const DstatQuartet &q, bool polarize,
                                           uint32_t wt, DstatAcc &a) {
    const uint32_t n1 = q.n[0], n2 = q.n[1], n3 = q.n[2], nO = q.n[3];
    if (polarize) {  // wave-uniform
        const bool flip = 2u * cO > nO, tie = 2u * cO == nO;
        c1 = flip ? n1 - c1 : c1;
        c2 = flip ? n2 - c2 : c2;
        c3 = flip ? n3 - c3 : c3;
        cO = flip ? nO - cO : cO;
        a.skip += tie;
        if (tie) c1 = c2 = c3 = cO = 0;  // all-zero counts add nothing below
    }
    const uint32_t rO = nO - cO, b = c3 * rO;
    const uint32_t ta = (n1 - c1) * c2, tb = c1 * (n2 - c2);
    const int32_t x = (int32_t)(c1 * n2) - (int32_t)(c2 * n1), y = (int32_t)(c3 * nO) - (int32_t)(cO * n3);
    const bool p2 = c2 * n3 >= c3 * n2;  // the donor of Martin's denominator: P2, else P3
    const int32_t dx = p2 ? -x : (int32_t)(c3 * n1) - (int32_t)(c1 * n3), dy = (int32_t)(p2 ? c2 * rO : b);
    a.inf += ((ta | tb) != 0u) & (b != 0u);
    if (WEIGHTED) {
        const uint64_t w = wt;
        a.abba += w * ((uint64_t)ta * b);
        a.baba += w * ((uint64_t)tb * b);
        a.f4 += (int64_t)w * ((int64_t)x * y);
        const int64_t fd = (int64_t)w * ((int64_t)dx * dy);
        a.fd2 += p2 ? fd : 0;
        a.fd3 += p2 ? 0 : fd;
    } else {
        a.abba += (uint64_t)ta * b;
        a.baba += (uint64_t)tb * b;
        a.f4 += (int64_t)x * y;
        a.fd2 += (int64_t)(p2 ? dx : 0) * dy;
        a.fd3 += (int64_t)(p2 ? 0 : dx) * dy;
    }
}

// grid = tiles, block = 256.  Dynamic LDS: the K masks, wps4 dwords each.  grp: the group's nq <= DSTAT_QG quartets.
// out: tile-major, DSTAT_QG x DSTAT_NV int64 per tile (the first nq are meaningful).
template <int K, bool WEIGHTED>
__global__ __launch_bounds__(256, 4) void dstat_tiles_kernel(const uint32_t *__restrict__ sb, const uint64_t *__restrict__ rare,
                                                             const ScanTile *__restrict__ tiles,
                                                             const uint32_t *__restrict__ masks /* K x wps */,
                                                             const uint32_t *__restrict__ pop_n /* K */, uint32_t wps, uint32_t G,
                                                             uint32_t r, const uint32_t *__restrict__ weights /* WEIGHTED */,
                                                             DstatGroup grp, uint32_t nq, int polarize, int64_t *__restrict__ out) {
    constexpr int NV = DSTAT_QG * DSTAT_NV;
    extern __shared__ __attribute__((aligned(16))) uint32_t mk_lds[];  // K x wps4
    pop_masks_to_lds<K>(mk_lds, masks, wps);
    __syncthreads();
    const ScanTile t = tiles[blockIdx.x];
    const TileBlocks tb = tile_blocks_of(t);
    const bool pol = polarize != 0;
    DstatAcc acc[DSTAT_QG];
    auto tally_counts = [&](const uint32_t (&c)[K], uint32_t wt) {
#pragma unroll
        for (int j = 0; j < DSTAT_QG; ++j) {
            if ((uint32_t)j >= nq) continue;  // wave-uniform: a short group
            const DstatQuartet &q = grp.q[j];
            dstat_site<WEIGHTED>(dstat_pick(c, q.p[0]), dstat_pick(c, q.p[1]), dstat_pick(c, q.p[2]), dstat_pick(c, q.p[3]), q, pol, wt,
                                 acc[j]);
        }
    };
    // the rare entries of the split index belong to unweighted matrices only: compiled out under WEIGHTED
    pop_stream_tile<K, !WEIGHTED>(
        sb, rare, t, tb, mk_lds, pop_n, wps, G, r, [&](const uint32_t (&c)[K], uint64_t s) { tally_counts(c, WEIGHTED ? weights[s] : 1u); },
        [&](const uint32_t (&c)[K]) { tally_counts(c, 1u); });
    tile_partials_store<NV>(tb, reinterpret_cast<uint64_t *>(out), [&](int i) -> uint64_t {
        const DstatAcc &a = acc[i / DSTAT_NV];
        switch (i % DSTAT_NV) {  // i is a constant once the caller's loop is unrolled
            case 0: return wave_sum_u64(a.abba);
            case 1: return wave_sum_u64(a.baba);
            case 2: return wave_sum_u64((uint64_t)a.f4);
            case 3: return wave_sum_u64((uint64_t)a.fd2);
            case 4: return wave_sum_u64((uint64_t)a.fd3);
            case 5: return wave_sum_u32(a.inf);
            default: return wave_sum_u32(a.skip);
        }
    });
}

// one thread per (window, quartet of the group): the window's tile range added up, the record's integers written
__global__ __launch_bounds__(128) void dstat_finalize_kernel(const int64_t *__restrict__ parts, const WinDesc *__restrict__ wins,
                                                             uint64_t n_windows, uint32_t nq, uint32_t q0, uint32_t n_quartets,
                                                             impop_dstat_stats *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_windows * nq) return;
    const uint64_t win = i / nq;
    const uint32_t j = (uint32_t)(i % nq);
    const WinDesc w = wins[win];
    int64_t s[DSTAT_NV] = {0, 0, 0, 0, 0, 0, 0};
    for (uint64_t t = w.t0; t < w.t1; ++t) {
        const int64_t *p = parts + (t * DSTAT_QG + j) * DSTAT_NV;
#pragma unroll
        for (int f = 0; f < DSTAT_NV; ++f) s[f] += p[f];
    }
    impop_dstat_stats o;
    o.n_sites = (uint32_t)w.n_sites;
    o.n_informative = (uint32_t)s[5];
    o.n_skipped = (uint32_t)s[6];
    o.flags = 0;
    o.abba = s[0];
    o.baba = s[1];
    o.f4_num = s[2];
    o.fd_den_p2 = s[3];
    o.fd_den_p3 = s[4];
    o.d = o.f4 = o.fd = 0.0;  // the host fills them in from the integers
    out[win * n_quartets + q0 + j] = o;
}

// IMPOP_DSTAT_TILE_BLOCKS=n (1..4096) overrides the tile size, so that tests reach many-tile windows on small matrices; it
// beats params->tile_blocks (0: the default)
static uint32_t dstat_tile_blocks(const impop_dstat_params *params) {
    const uint32_t e = env_tile_blocks("IMPOP_DSTAT_TILE_BLOCKS");
    return e ? e : std::min<uint32_t>(params->tile_blocks, 4096u);
}

}  // namespace impop

using namespace impop;

IMPOP_API int impop_dstat_scan(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows,
                               const uint64_t *masks, uint32_t n_pop, const uint32_t *quartets, uint32_t n_quartets,
                               const impop_dstat_params *params, impop_dstat_stats *out_host) {
    static_assert(sizeof(impop_dstat_stats) == 80 && sizeof(impop_dstat_params) == 16 && sizeof(DstatQuartet) == 32, "ABI layout");
    const char *fn = "impop_dstat_scan";
    REQUIRE(ctx && m && params, "%s: NULL argument", fn);
    REQUIRE(params->struct_size == sizeof(impop_dstat_params), "impop_dstat_params.struct_size mismatch");
    REQUIRE(m->device == ctx->device, "%s: matrix lives on device %d, context on %d", fn, m->device, ctx->device);
    REQUIRE(n_pop >= 4 && n_pop <= 8, "%s: n_pop must be 4..8 (got %u)", fn, n_pop);
    REQUIRE(masks, "%s: masks is NULL", fn);
    REQUIRE(n_quartets >= 1 && n_quartets <= IMPOP_DSTAT_MAX_QUARTETS && quartets, "%s: n_quartets must be 1..%u (got %u)", fn,
            IMPOP_DSTAT_MAX_QUARTETS, n_quartets);
    REQUIRE(m->g.n_hap <= 65535, "%s: n_hap > 65535 not supported", fn);
    const uint32_t wps = m->g.wps, K = n_pop, Q = n_quartets;
    PopPanel panel;
    pop_panel_pack(m, masks, K, panel);
    const std::vector<uint32_t> &mk = panel.mk, &nk = panel.nk;
    for (uint32_t k = 0; k < K; ++k) REQUIRE(nk[k] > 0, "%s: population %u is empty", fn, k);
    std::vector<DstatQuartet> qs(Q);
    for (uint32_t q = 0; q < Q; ++q) {
        for (int a = 0; a < 4; ++a) {
            const uint32_t p = quartets[4 * q + a];
            REQUIRE(p < K, "%s: quartet %u: population index %u outside the %u populations", fn, q, p, K);
            qs[q].p[a] = p;
            qs[q].n[a] = nk[p];
        }
        for (int a = 0; a < 4; ++a)
            for (int b = a + 1; b < 4; ++b)
                for (uint32_t j = 0; j < wps; ++j)
                    REQUIRE((mk[(size_t)qs[q].p[a] * wps + j] & mk[(size_t)qs[q].p[b] * wps + j]) == 0u,
                            "%s: quartet %u: populations %u and %u share a haplotype (the four populations of a quartet must be disjoint)",
                            fn, q, qs[q].p[a], qs[q].p[b]);
    }
    int rc = check_windows(fn, m, windows, windows ? n_windows : 0);
    if (rc) return rc;
    if (!n_windows) return IMPOP_OK;
    REQUIRE(windows && out_host, "%s: NULL windows/out", fn);
    // no sum can wrap: every term is at most n1 nO max(n2, n3)^2 in magnitude, a window adds at most its weight sum of them
    uint64_t w_max = 0, w_arg = 0;
    for (uint64_t i = 0; i < n_windows; ++i) {
        const uint64_t W = window_W(m, windows[i].site_begin, windows[i].site_end);
        if (W > w_max) { w_max = W; w_arg = i; }
    }
    for (uint32_t q = 0; q < Q; ++q) {
        const uint64_t mx = std::max(qs[q].n[1], qs[q].n[2]);
        const unsigned __int128 bound = (unsigned __int128)((uint64_t)qs[q].n[0] * qs[q].n[3]) * (mx * mx) * w_max;
        if (bound >= ((unsigned __int128)1 << 62)) {
            set_error("%s: quartet %u (population sizes %u, %u, %u, %u) over window %llu (weight sum %llu): n1 nO max(n2, n3)^2 W is not "
                      "below 2^62, the sums could wrap; split the window",
                      fn, q, qs[q].n[0], qs[q].n[1], qs[q].n[2], qs[q].n[3], (unsigned long long)w_arg, (unsigned long long)w_max);
            return IMPOP_E_UNSUPPORTED;
        }
    }

    HIP_TRY(hipSetDevice(ctx->device));
    ScanRoute rt;
    rc = scan_route(fn, ctx, m, windows, n_windows, dstat_tile_blocks(params), rt);
    if (rc) return rc;
    const size_t nt = rt.tiles.size();
    PopPanelDev dev;
    int64_t *dp = nullptr;
    impop_dstat_stats *d_out = nullptr;
    rc = pop_panel_upload(ctx, rt, panel, dev, [&](Layout &L) {
        L.sub(dp, std::max<size_t>(nt, 1) * DSTAT_QG * DSTAT_NV);
        L.sub(d_out, n_windows * Q);
    });
    if (rc) return rc;
    const uint32_t *weights = m->d_wt && !rt.indexed ? m->d_wt : nullptr;  // weighted matrices stream their rows
    const int polarize = params->polarize != 0;
    uint64_t launches = 0;
    // the quartet list in groups of DSTAT_QG: the same tiles, the partials reused (the launches of a stream run in order)
    for (uint32_t q0 = 0; q0 < Q; q0 += DSTAT_QG) {
        const uint32_t nq = std::min<uint32_t>(DSTAT_QG, Q - q0);
        DstatGroup grp;
        for (uint32_t j = 0; j < (uint32_t)DSTAT_QG; ++j) grp.q[j] = qs[q0 + (j < nq ? j : 0)];  // a short group repeats its first quartet
        if (nt) {
            rc = timed(ctx, ctx->timers[impop_ctx::T_DSTAT], [&] {
                return pop_dispatch_k<4>(K, [&](auto k) {
                    return weights ? pop_launch(dstat_tiles_kernel<k.value, true>, K, ctx->stream, m, rt, dev, weights, grp, nq, polarize, dp)
                                   : pop_launch(dstat_tiles_kernel<k.value, false>, K, ctx->stream, m, rt, dev, weights, grp, nq, polarize, dp);
                });
            });
            if (rc) return rc;
            ++launches;
        }
        const uint64_t items = n_windows * nq;
        hipLaunchKernelGGL(dstat_finalize_kernel, dim3((uint32_t)((items + 127) / 128)), dim3(128), 0, ctx->stream, dp,
                           (const WinDesc *)dev.wins, n_windows, nq, q0, Q, d_out);
        HIP_TRY(hipGetLastError());
        ++launches;
    }
    HIP_TRY(hipMemcpyAsync(out_host, d_out, n_windows * Q * sizeof(impop_dstat_stats), hipMemcpyDeviceToHost, ctx->stream));
    rc = ctx_err_fetch(ctx);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    rc = ctx_err_result(ctx, fn);
    if (rc) return rc;
    const double nan = __builtin_nan("");
    for (uint64_t i = 0; i < n_windows; ++i)
        for (uint32_t q = 0; q < Q; ++q) {
            impop_dstat_stats &o = out_host[i * Q + q];
            const uint64_t n1 = qs[q].n[0], n2 = qs[q].n[1], n3 = qs[q].n[2], nO = qs[q].n[3];
            const int64_t num = o.abba - o.baba, den = o.abba + o.baba;
            o.d = den == 0 ? nan : (double)num / (double)den;
            o.f4 = (double)o.f4_num / (double)(n1 * n2 * n3 * nO);
            const double fd_den = (double)o.fd_den_p2 / (double)(n1 * n2 * n2 * nO) + (double)o.fd_den_p3 / (double)(n1 * n3 * n3 * nO);
            o.fd = fd_den == 0.0 ? nan : ((double)num / (double)(n1 * n2 * n3 * nO)) / fd_den;
        }
    if (trace_on()) {
        fprintf(stderr, "[impop_dstat_scan] route=%s windows=%llu tiles=%llu quartets=%u launches=%llu bytes_streamed=%llu\n",
                rt.split ? "indexed+rare" : rt.indexed ? "indexed" : m->compact ? "compact" : "dense", (unsigned long long)n_windows,
                (unsigned long long)nt, Q, (unsigned long long)launches, (unsigned long long)rt.bytes_streamed);
        fflush(stderr);
    }
    return IMPOP_OK;
}

IMPOP_API int impop_ctx_dstat_elapsed(impop_ctx *ctx, double *total_ms, uint64_t *launches) {
    REQUIRE(ctx, "impop_ctx_dstat_elapsed: ctx is NULL");
    return ctx_timers_elapsed(ctx, impop_ctx::T_DSTAT, 1, 0, total_ms, launches);
}
