// ldscan.hip — impop_ld_scan: linkage disequilibrium between the sites of every window (Kelly's ZnS, mean |D'|, the Kim-Nielsen
// omega) from the site-major rows alone.  A site's row holds the haplotypes as bits, so a site pair costs wps ANDs and popcounts.
//
// Windows are mapped straight onto d_sb, which holds every row of the matrix whatever index was built beside it (a compacted
// matrix: onto its kept sites; the dropped ones are monomorphic and never qualify), so a record cannot depend on the upload's
// keep flags.  Per chunk of windows, three launches:
//   1. ld_select_kernel  the qualifying mask of every 64-site block of a window            (ld_select.h, shared with recomb.hip)
//   2. ld_gather_kernel  the used sites' rows ANDed with P, their c and their original coordinate go to the chunk's scratch at
//                        [window][k]                                                            (ld_select.h)
//   3. ld_pairs_kernel   one workgroup per window: the lane that owns site t runs k = 0..m-1 over broadcast rows and adds r2 into
//                        a_t while k < t and into b_t while k > t, |D'| into dp_t while k < t — every pair is evaluated twice and
//                        nothing is accumulated across lanes, so the doubles do not depend on scheduling.  One lane then runs the
//                        sequential prefix L, suffix R and the omega search, and stores the record.
// Operation order of every double: include/impop_hip.h, impop_ld_scan.
#include <string.h>

#include <algorithm>
#include <vector>

#include "device_utils.h"
#include "internal.h"
#include "ld_select.h"
#include "sb64.h"
#include "scan_route.h"
#include "win_chunks.h"

namespace impop {

// the used rows of a window are staged in LDS up to this many bytes (465 haplotypes x 512 sites: 32 KB); else read from scratch
constexpr size_t LD_LDS_ROW_BYTES = 64 * 1024;
static_assert(IMPOP_LD_MAX_N <= 4096u, "num^2 and den stay below 2^53 only for n <= 4096");
static_assert(IMPOP_LD_MAX_SITES <= LD_GATHER_LDS_SITES, "the gather keeps this call's site list in LDS");

// grid = windows of the chunk.  Dynamic LDS: a, b, dp (8 max_sites each) | c (4 max_sites) | 4 counters | LDS_ROWS: the rows,
// one every wps | 1 dwords (an odd stride: the lanes' own rows fall on different banks).
template <bool LDS_ROWS>
__global__ __launch_bounds__(LD_T) void ld_pairs_kernel(const uint32_t *__restrict__ rows, const uint32_t *__restrict__ cs,
                                                        const uint32_t *__restrict__ qm, const LdWin *__restrict__ wins, uint32_t wps,
                                                        uint32_t max_sites, uint32_t nP, impop_ld_stats *__restrict__ rec) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ld_lds[];
    double *a = reinterpret_cast<double *>(ld_lds), *b = a + max_sites, *dp = b + max_sites;
    uint32_t *cl = reinterpret_cast<uint32_t *>(dp + max_sites), *cnt = cl + max_sites, *lrows = cnt + 4;
    const uint32_t tid = threadIdx.x, win = blockIdx.x;
    const uint32_t q = qm[2 * win], m = qm[2 * win + 1];
    const uint64_t o = (uint64_t)win * max_sites;
    const uint32_t *grow = rows + o * wps;
    const uint32_t stride = LDS_ROWS ? (wps | 1u) : wps;
    if (LDS_ROWS)
        for (uint32_t idx = tid; idx < m * wps; idx += LD_T) lrows[(idx / wps) * stride + idx % wps] = grow[idx];
    for (uint32_t k = tid; k < m; k += LD_T) cl[k] = cs[o + k];
    if (tid == 0) cnt[0] = cnt[1] = 0u;
    __syncthreads();
    const int64_t n = nP;
    uint32_t perfect = 0, complete = 0;
    for (uint32_t t = tid; t < m; t += LD_T) {
        const int64_t ct = cl[t];
        double at = 0.0, bt = 0.0, dt = 0.0;
        for (uint32_t k = 0; k < m; ++k) {
            uint32_t n11 = 0;
            if (LDS_ROWS) {
                for (uint32_t j = 0; j < wps; ++j) n11 += __popc(lrows[t * stride + j] & lrows[k * stride + j]);
            } else {
                for (uint32_t j = 0; j < wps; ++j) n11 += __popc(grow[(uint64_t)t * wps + j] & grow[(uint64_t)k * wps + j]);
            }
            const int64_t ck = cl[k];
            const int64_t num = n * (int64_t)n11 - ct * ck;
            const int64_t den = ct * (n - ct) * (ck * (n - ck));
            const double r2 = (double)(num * num) / (double)den;
            if (k < t) {
                at += r2;
                double d = 0.0;
                if (num != 0) {
                    const int64_t x = num > 0 ? ct * (n - ck) : ct * ck, y = num > 0 ? (n - ct) * ck : (n - ct) * (n - ck);
                    const int64_t dmax = x < y ? x : y, an = num < 0 ? -num : num;
                    d = (double)an / (double)dmax;
                    complete += an == dmax;
                }
                dt += d;
                perfect += num * num == den;
            } else if (k > t) {
                bt += r2;
            }
        }
        a[t] = at;
        b[t] = bt;
        dp[t] = dt;
    }
    if (perfect) atomicAdd(&cnt[0], perfect);
    if (complete) atomicAdd(&cnt[1], complete);
    __syncthreads();
    if (tid != 0) return;
    // a[l] <- L(l), b[l] <- R(l); L(m) = sum_r2 and R(m) = 0 are not stored: no split uses them
    double run = 0.0;
    for (uint32_t j = 0; j < m; ++j) {
        const double aj = a[j];
        a[j] = run;
        run += aj;
    }
    const double sum_r2 = run;
    run = 0.0;
    for (uint32_t j = m; j-- > 0;) {
        run += b[j];
        b[j] = run;
    }
    double sum_dp = 0.0;
    for (uint32_t j = 0; j < m; ++j) sum_dp += dp[j];
    double best = 0.0;
    uint32_t split = 0;
    for (uint32_t l = 2; l + 2 <= m; ++l) {
        const double cross = (sum_r2 - a[l]) - b[l];
        if (!(cross > 0.0)) continue;
        const uint64_t within = (uint64_t)l * (l - 1) / 2 + (uint64_t)(m - l) * (m - l - 1) / 2, between = (uint64_t)l * (m - l);
        const double om = ((a[l] + b[l]) / (double)within) / (cross / (double)between);
        if (split == 0 || om > best) {
            best = om;
            split = l;
        }
    }
    impop_ld_stats out;
    out.n_members = nP;
    out.n_sites = wins[win].n_sites;
    out.n_qualifying = q;
    out.n_used = m;
    out.n_perfect = cnt[0];
    out.n_complete = cnt[1];
    out.omega_split = split;
    out.reserved = 0;
    out.sum_r2 = sum_r2;
    out.sum_dprime = sum_dp;
    const uint64_t pairs = (uint64_t)m * (m > 0 ? m - 1 : 0) / 2;
    out.zns = m < 2 ? 0.0 : sum_r2 / (double)pairs;
    out.mean_dprime = m < 2 ? 0.0 : sum_dp / (double)pairs;
    out.omega_max = best;
    rec[win] = out;
}

}  // namespace impop

using namespace impop;

IMPOP_API int impop_ld_scan(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows, const uint64_t *mask_p,
                            const impop_ld_params *params, impop_ld_stats *out_host, uint64_t *used_sites) {
    static_assert(sizeof(impop_ld_stats) == 72 && sizeof(impop_ld_params) == 24 && sizeof(LdWin) == 40, "ABI layout");
    const char *fn = "impop_ld_scan";
    REQUIRE(ctx && m && params, "%s: NULL argument", fn);
    REQUIRE(params->struct_size == sizeof(impop_ld_params), "impop_ld_params.struct_size mismatch");
    REQUIRE(m->device == ctx->device, "%s: matrix lives on device %d, context on %d", fn, m->device, ctx->device);
    const uint32_t n = m->g.n_hap, wps = m->g.wps;
    const MemberSet P = member_set(mask_p, n, wps);
    const uint32_t nP = P.size();
    REQUIRE(nP > 0, "%s: the mask selects no haplotype", fn);
    REQUIRE(params->min_mac >= 1, "%s: min_mac must be at least 1", fn);
    const uint32_t max_sites = params->max_sites ? params->max_sites : 512u;
    REQUIRE(max_sites >= 4 && max_sites <= IMPOP_LD_MAX_SITES, "%s: max_sites %u outside 4..%u", fn, max_sites, (uint32_t)IMPOP_LD_MAX_SITES);
    int rc = check_windows(fn, m, windows, windows ? n_windows : 0);
    if (rc) return rc;
    if (nP > IMPOP_LD_MAX_N) {
        set_error("%s: %u members exceed the exact-arithmetic limit (%u)", fn, nP, (uint32_t)IMPOP_LD_MAX_N);
        return IMPOP_E_UNSUPPORTED;
    }
    if (!n_windows) return IMPOP_OK;
    REQUIRE(windows && out_host, "%s: NULL windows/out", fn);
    std::vector<impop_window> mapped;
    map_windows(m, windows, n_windows, mapped);
    if ((rc = check_window_weights(fn, m, windows, n_windows))) return rc;

    // a window's device bytes: its gathered rows, their c and coordinates, the record, the descriptor, (q, m), a mask per block
    const uint64_t per_win = (uint64_t)max_sites * (4ull * wps + 12) + sizeof(impop_ld_stats) + sizeof(LdWin) + 8;
    std::vector<uint64_t> nb(n_windows);  // the 64-site blocks a window touches
    uint64_t bytes_streamed = 0;
    for (uint64_t i = 0; i < n_windows; ++i) {
        const uint64_t s0 = mapped[i].site_begin, s1 = mapped[i].site_end;
        nb[i] = ld_blocks(s0, s1);
        bytes_streamed += nb[i] * 256ull * wps;
    }
    const std::vector<WinChunk> chunks =
        cut_windows(n_windows, chunk_budget(params->max_chunk_bytes), 0, [&](size_t, uint64_t i) { return per_win + nb[i] * 8; });
    const size_t max_wins = max_over(chunks, [](const WinChunk &c) { return c.w_end - c.w_begin; }),
                 max_blocks = max_over(chunks, [&](const WinChunk &c) {
                     uint64_t sum = 0;
                     for (uint64_t i = c.w_begin; i < c.w_end; ++i) sum += nb[i];
                     return sum;
                 });
    REQUIRE(max_wins < 0x7FFFFFFFull, "%s: a chunk of %zu windows exceeds one launch", fn, max_wins);

    // device: P as dwords | windows (up, through the page-locked staging with the same offsets) | records (down, staged) |
    // (q, m) per window | qualifying masks | gathered rows, their c, their coordinates
    Carve L;
    const size_t o_pbits = L.take<uint32_t>(wps), o_wins = L.take<LdWin>(max_wins), o_rec = L.take<impop_ld_stats>(max_wins),
                 staged = L.total(), o_qm = L.take<uint32_t>(2 * max_wins), o_qmask = L.take<uint64_t>(max_blocks),
                 o_rows = L.take<uint32_t>(max_wins * max_sites * wps), o_cs = L.take<uint32_t>(max_wins * max_sites),
                 o_coords = L.take<uint64_t>(max_wins * max_sites);
    HIP_TRY(hipSetDevice(ctx->device));
    void *d = nullptr, *pin = nullptr;
    rc = ctx_scratch(ctx, L.total(), &d);
    if (rc) return rc;
    rc = ctx_pinned(ctx, staged, &pin);
    if (rc) return rc;
    const ChunkRun run{ctx, fn, (char *)d, (char *)pin};
    char *dc = run.dc, *hc = run.hc;
    memcpy(hc + o_pbits, P.bits.data(), (size_t)wps * 4);
    if ((rc = run.up(o_pbits, o_pbits + (size_t)wps * 4))) return rc;

    const size_t lds_rows = (size_t)max_sites * (wps | 1u) * 4;
    const bool rows_in_lds = lds_rows <= LD_LDS_ROW_BYTES;
    const size_t lds_pairs = (size_t)max_sites * 28 + 16 + (rows_in_lds ? lds_rows : 0);
    if ((rc = rows_in_lds ? lds_opt_in(ld_pairs_kernel<true>, lds_pairs) : lds_opt_in(ld_pairs_kernel<false>, lds_pairs))) return rc;

    const uint32_t *d_pbits = (const uint32_t *)(dc + o_pbits);
    const LdWin *d_wins = (const LdWin *)(dc + o_wins);
    impop_ld_stats *d_rec = (impop_ld_stats *)(dc + o_rec);
    uint32_t *d_qm = (uint32_t *)(dc + o_qm), *d_rows = (uint32_t *)(dc + o_rows), *d_cs = (uint32_t *)(dc + o_cs);
    uint64_t *d_qmask = (uint64_t *)(dc + o_qmask), *d_coords = (uint64_t *)(dc + o_coords);
    LdWin *h_wins = (LdWin *)(hc + o_wins);
    EventPairs *timer = ctx->timers + impop_ctx::T_LD;
    uint64_t launches = 0, qualifying = 0, used = 0;
    for (const WinChunk &c : chunks) {
        const size_t cnt = c.w_end - c.w_begin;
        uint64_t n_blocks = 0, longest = 0;  // blocks of all the chunk's windows / of its longest one
        for (size_t k = 0; k < cnt; ++k) {
            const uint64_t i = c.w_begin + k;
            h_wins[k] = LdWin{mapped[i].site_begin, mapped[i].site_end, n_blocks, (uint64_t)k * max_sites,
                              (uint32_t)window_W(m, windows[i].site_begin, windows[i].site_end), max_sites};
            n_blocks += nb[i];
            longest = std::max(longest, nb[i]);
        }
        if ((rc = run.up(o_wins, o_wins + cnt * sizeof(LdWin)))) return rc;
        const uint32_t slices = ld_select_slices(longest);
        if ((rc = run.timed(timer[0], [&] {
            hipLaunchKernelGGL(ld_select_kernel, dim3((uint32_t)cnt, slices), dim3(LD_T), 0, ctx->stream, m->d_sb, d_wins, wps, m->g.G, m->g.r,
                               d_pbits, nP, params->min_mac, d_qmask);
        }))) return rc;
        if ((rc = run.timed(timer[1], [&] {
            hipLaunchKernelGGL(ld_gather_kernel, dim3((uint32_t)cnt), dim3(LD_T), 0, ctx->stream, m->d_sb, d_wins, wps, m->g.G, m->g.r, d_pbits,
                               m->compact ? m->d_pos : nullptr, max_sites, d_qmask, d_rows, d_cs, d_coords, d_qm, nullptr, ctx->d_err,
                               DEV_ERR_LDSCAN);
        }))) return rc;
        if ((rc = run.timed(timer[2], [&] {
            if (rows_in_lds)
                hipLaunchKernelGGL(ld_pairs_kernel<true>, dim3((uint32_t)cnt), dim3(LD_T), lds_pairs, ctx->stream, d_rows, d_cs, d_qm, d_wins,
                                   wps, max_sites, nP, d_rec);
            else
                hipLaunchKernelGGL(ld_pairs_kernel<false>, dim3((uint32_t)cnt), dim3(LD_T), lds_pairs, ctx->stream, d_rows, d_cs, d_qm, d_wins,
                                   wps, max_sites, nP, d_rec);
        }))) return rc;
        launches += 3;
        if (used_sites)
            HIP_TRY(hipMemcpyAsync(used_sites + c.w_begin * max_sites, d_coords, cnt * max_sites * 8, hipMemcpyDeviceToHost, ctx->stream));
        if ((rc = run.finish(o_rec, o_rec + cnt * sizeof(impop_ld_stats)))) return rc;
        const impop_ld_stats *rv = (const impop_ld_stats *)(hc + o_rec);
        for (size_t k = 0; k < cnt; ++k) {
            out_host[c.w_begin + k] = rv[k];
            qualifying += rv[k].n_qualifying;
            used += rv[k].n_used;
        }
    }
    if (trace_on()) {
        fprintf(stderr, "[impop_ld_scan] route=%s windows=%llu chunks=%llu launches=%llu qualifying=%llu used=%llu bytes_streamed=%llu\n",
                m->compact ? "compact" : "dense", (unsigned long long)n_windows, (unsigned long long)chunks.size(),
                (unsigned long long)launches, (unsigned long long)qualifying, (unsigned long long)used,
                (unsigned long long)(bytes_streamed + used * 4ull * wps));
        fflush(stderr);
    }
    return IMPOP_OK;
}

IMPOP_API int impop_ctx_ld_elapsed(impop_ctx *ctx, double kernel_ms[3], uint64_t *chunks) {
    REQUIRE(ctx && kernel_ms, "impop_ctx_ld_elapsed: NULL argument");
    return ctx_timers_elapsed(ctx, impop_ctx::T_LD, 3, 2, kernel_ms, chunks);
}
