// recomb.hip — impop_recomb_scan: the four-gamete test between all used sites of every window, and from it Hudson & Kaplan's
// R_min, four-gamete blocks and Wall's B and Q.  A site's row holds the members as bits, so a site pair costs wps ANDs and
// popcounts; everything the device writes is an integer (contract: include/impop_hip.h, impop_recomb_scan).
//
// Site selection is impop_ld_scan's (ld_select.h).  A window's slots in the chunk's scratch number cap = min(max_sites, its sites)
// and start at the prefix of the windows before it, so that one chromosome-arm window among thousands of short ones costs what it
// holds, not max_sites per window.  Per chunk of windows, four launches:
//   1. ld_select_kernel      the qualifying mask of every 64-site block                                       (streams the rows)
//   2. ld_gather_kernel      the used sites' masked rows, carrier counts, coordinates; the site list lives in scratch above
//                            1024 sites                                                                      (reads m rows)
//   3. recomb_pairs_kernel   grid = (window, tile of 256 sites j) items, enumerated on the host from cap; items past a window's
//                            m leave at once.  A lane owns site j, its row in registers up to 32 dwords; the sites i < j go
//                            through LDS 256 at a time and are read as broadcasts.  Per site: the nearest incompatible site on
//                            the left (max), how many (count), the first congruent site (min) — integers, any order gives the
//                            same bytes.  A tile at position T of a window reads T + 1 staged blocks: work is the triangle.
//   4. recomb_finish_kernel  one wave per window: the lanes stage 64 sites' results, lane 0 runs recomb_math.h over them.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "chunk_run.h"
#include "device_utils.h"
#include "internal.h"
#include "ld_select.h"
#include "recomb_math.h"
#include "scan_route.h"
#include "win_chunks.h"

namespace impop {

constexpr uint32_t RC_T = 256;  // sites of a tile = threads of the pair kernel's workgroup

struct RecombItem {
    uint32_t win, tile;
};

// WR > 0: a row has at most WR dwords and is kept in registers, LDS rows are padded to WR with zeros; WR == 0: any wps, the
// lane's own row is read from the scratch.  Dynamic LDS: RC_T rows of (WR ? WR : wps) dwords | RC_T carrier counts.
template <uint32_t WR>
__global__ __launch_bounds__(RC_T) void recomb_pairs_kernel(const uint32_t *__restrict__ rows, const uint32_t *__restrict__ cs,
                                                            const uint32_t *__restrict__ qm, const LdWin *__restrict__ wins,
                                                            const RecombItem *__restrict__ items, uint32_t wps, uint32_t nP,
                                                            impop_recomb_site *__restrict__ site_tab) {
    extern __shared__ __attribute__((aligned(16))) uint32_t rc_lds[];
    const RecombItem it = items[blockIdx.x];
    const uint32_t m = qm[2 * it.win + 1], j0 = it.tile * RC_T, tid = threadIdx.x;
    if (j0 >= m) return;  // the whole workgroup: the window holds fewer sites than its slots
    const LdWin w = wins[it.win];
    const uint32_t *grow = rows + w.row_off * wps, *gcs = cs + w.row_off;
    const uint32_t stride = WR ? WR : wps;
    uint32_t *lrow = rc_lds, *lc = rc_lds + RC_T * stride;
    const uint32_t j = j0 + tid;
    const bool live = j < m;
    uint32_t mine[WR ? WR : 1];
    if (WR) {
#pragma unroll
        for (uint32_t u = 0; u < WR; ++u) mine[u] = live && u < wps ? grow[(uint64_t)j * wps + u] : 0u;
    }
    const uint32_t *own = grow + (uint64_t)(live ? j : 0u) * wps;
    const uint32_t cj = live ? gcs[j] : 0u;
    uint32_t left1 = 0, n_left = 0, rep = j;
    for (uint32_t k0 = 0; k0 <= j0; k0 += RC_T) {
        const uint32_t kn = m - k0 < RC_T ? m - k0 : RC_T;
        __syncthreads();  // the block before this one has been read
        for (uint32_t idx = tid; idx < kn * stride; idx += RC_T) {
            const uint32_t k = idx / stride, u = idx % stride;
            lrow[idx] = u < wps ? grow[(uint64_t)(k0 + k) * wps + u] : 0u;
        }
        if (tid < kn) lc[tid] = gcs[k0 + tid];
        __syncthreads();
        if (!live) continue;
        const uint32_t kend = j - k0 < kn ? j - k0 : kn;  // sites left of j only
        for (uint32_t k = 0; k < kend; ++k) {
            uint32_t n11 = 0;
            if (WR) {
#pragma unroll
                for (uint32_t u = 0; u < WR; ++u) n11 += __popc(mine[u] & lrow[k * WR + u]);
            } else {
                for (uint32_t u = 0; u < wps; ++u) n11 += __popc(own[u] & lrow[k * stride + u]);
            }
            const uint32_t ck = lc[k];
            const uint32_t n10 = ck - n11, n01 = cj - n11, n00 = nP + n11 - ck - cj;
            if (n11 && n10 && n01 && n00) {
                left1 = k0 + k + 1;
                ++n_left;
            }
            if (((n10 | n01) == 0u || (n11 | n00) == 0u) && k0 + k < rep) rep = k0 + k;
        }
    }
    if (live) {
        impop_recomb_site out;
        out.left1 = left1;
        out.n_left = n_left;
        out.rep = rep;
        out.carriers = cj;
        site_tab[w.row_off + j] = out;
    }
}

// grid = windows of the chunk, one wave each
__global__ __launch_bounds__(64) void recomb_finish_kernel(const impop_recomb_site *__restrict__ site_tab, const uint64_t *__restrict__ coords,
                                                           const uint32_t *__restrict__ qm, const LdWin *__restrict__ wins, uint32_t nP,
                                                           impop_recomb_stats *__restrict__ rec, uint32_t *__restrict__ err) {
    __shared__ uint32_t seen[RECOMB_MAX_SITES / 32];
    __shared__ impop_recomb_site buf[64];
    const uint32_t lane = threadIdx.x, win = blockIdx.x;
    const uint32_t q = qm[2 * win], m = qm[2 * win + 1] <= RECOMB_MAX_SITES ? qm[2 * win + 1] : RECOMB_MAX_SITES;
    const LdWin w = wins[win];
    const impop_recomb_site *tab = site_tab + w.row_off;
    for (uint32_t i = lane; i < recomb_seen_words(m); i += 64) seen[i] = 0u;
    RecombState st = recomb_start();
    for (uint32_t j0 = 0; j0 < m; j0 += 64) {
        __syncthreads();
        if (j0 + lane < m) buf[lane] = tab[j0 + lane];
        __syncthreads();
        if (lane == 0) {
            const uint32_t cnt = m - j0 < 64u ? m - j0 : 64u;
            for (uint32_t t = 0; t < cnt; ++t) recomb_step(st, j0 + t, buf[t].left1, buf[t].n_left, buf[t].rep, seen);
        }
    }
    if (lane != 0) return;
    recomb_end(st, m);
    if (st.rmin > st.n_positive || qm[2 * win + 1] != m) atomicOr(err, DEV_ERR_RECOMB);
    impop_recomb_stats out;
    out.n_members = nP;
    out.n_sites = w.n_sites;
    out.n_qualifying = q;
    out.n_used = m;
    out.rmin = st.rmin;
    out.n_incompatible_adjacent = st.n_adjacent;
    out.n_blocks = st.n_blocks;
    out.longest_block_sites = st.longest;
    out.n_congruent_adjacent = st.n_congruent_adjacent;
    out.n_congruent_partitions = st.n_congruent_partitions;
    out.n_partitions = st.n_partitions;
    out.reserved = 0;
    out.n_incompatible = st.n_incompatible;
    out.longest_block_begin = m ? coords[w.row_off + st.longest_first] : 0ull;
    out.longest_block_end = m ? coords[w.row_off + st.longest_last] : 0ull;
    out.four_gamete_fraction = out.wall_b = out.wall_q = 0.0;  // the host's, from the integers
    rec[win] = out;
}

// the record's three doubles: one division of exact values each, NaN where the denominator is 0
static void recomb_doubles(impop_recomb_stats &r) {
    const uint64_t m = r.n_used, pairs = m * (m ? m - 1 : 0) / 2;
    r.four_gamete_fraction = pairs ? (double)r.n_incompatible / (double)pairs : NAN;
    r.wall_b = m > 1 ? (double)r.n_congruent_adjacent / (double)(m - 1) : NAN;
    r.wall_q = m > 0 ? (double)((uint64_t)r.n_congruent_adjacent + r.n_congruent_partitions) / (double)m : NAN;
}

template <uint32_t WR>
static int launch_recomb_pairs(impop_ctx *ctx, uint32_t n_items, size_t lds, const uint32_t *rows, const uint32_t *cs, const uint32_t *qm,
                               const LdWin *wins, const RecombItem *items, uint32_t wps, uint32_t nP, impop_recomb_site *tab) {
    const int rc = lds_opt_in(recomb_pairs_kernel<WR>, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(recomb_pairs_kernel<WR>, dim3(n_items), dim3(RC_T), lds, ctx->stream, rows, cs, qm, wins, items, wps, nP, tab);
    return IMPOP_OK;
}

}  // namespace impop

using namespace impop;

static_assert(IMPOP_RECOMB_MAX_N == RECOMB_MAX_N && IMPOP_RECOMB_MAX_SITES == RECOMB_MAX_SITES, "the header's constants");

IMPOP_API int impop_recomb_scan(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows,
                                const uint64_t *mask_p, const impop_recomb_params *params, impop_recomb_stats *out_host,
                                uint64_t *used_sites, impop_recomb_site *site_table) {
    static_assert(sizeof(impop_recomb_stats) == 96 && sizeof(impop_recomb_params) == 24 && sizeof(impop_recomb_site) == 16 &&
                  sizeof(RecombItem) == 8, "ABI layout");
    const char *fn = "impop_recomb_scan";
    REQUIRE(ctx && m && params, "%s: NULL argument", fn);
    REQUIRE(params->struct_size == sizeof(impop_recomb_params), "impop_recomb_params.struct_size mismatch");
    REQUIRE(m->device == ctx->device, "%s: matrix lives on device %d, context on %d", fn, m->device, ctx->device);
    const uint32_t n = m->g.n_hap, wps = m->g.wps;
    const MemberSet P = member_set(mask_p, n, wps);
    const uint32_t nP = P.size();
    REQUIRE(nP > 0, "%s: the mask selects no haplotype", fn);
    REQUIRE(params->min_mac >= 1, "%s: min_mac must be at least 1", fn);
    const uint32_t max_sites = params->max_sites ? params->max_sites : 4096u;
    REQUIRE(max_sites >= 2 && max_sites <= IMPOP_RECOMB_MAX_SITES, "%s: max_sites %u outside 2..%u", fn, max_sites,
            (uint32_t)IMPOP_RECOMB_MAX_SITES);
    int rc = check_windows(fn, m, windows, windows ? n_windows : 0);
    if (rc) return rc;
    if (nP > IMPOP_RECOMB_MAX_N) {
        set_error("%s: %u members exceed the limit (%u)", fn, nP, (uint32_t)IMPOP_RECOMB_MAX_N);
        return IMPOP_E_UNSUPPORTED;
    }
    if (!n_windows) return IMPOP_OK;
    REQUIRE(windows && out_host, "%s: NULL windows/out", fn);
    std::vector<impop_window> mapped;
    map_windows(m, windows, n_windows, mapped);
    if ((rc = check_window_weights(fn, m, windows, n_windows))) return rc;

    // a slot's device bytes: the gathered row, its c, its coordinate, its place in the site list, its site_table row; a window's:
    // the record, the descriptor, (q, m), a mask per block, an item per tile of its slots
    const uint64_t per_slot = 4ull * wps + 4 + 8 + 8 + sizeof(impop_recomb_site);
    const uint64_t per_win = sizeof(impop_recomb_stats) + sizeof(LdWin) + 8;
    std::vector<uint64_t> nb(n_windows);    // the 64-site blocks a window touches
    std::vector<uint32_t> cap(n_windows);   // its slots
    uint64_t bytes_streamed = 0;
    for (uint64_t i = 0; i < n_windows; ++i) {
        const uint64_t s0 = mapped[i].site_begin, s1 = mapped[i].site_end;
        nb[i] = ld_blocks(s0, s1);
        cap[i] = (uint32_t)std::min<uint64_t>(s1 > s0 ? s1 - s0 : 0, max_sites);
        bytes_streamed += nb[i] * 256ull * wps;
    }
    auto tiles_of = [](uint64_t sites) { return (sites + RC_T - 1) / RC_T; };
    const std::vector<WinChunk> chunks = cut_windows(n_windows, chunk_budget(params->max_chunk_bytes), 0, [&](size_t, uint64_t i) {
        return per_win + nb[i] * 8 + cap[i] * per_slot + tiles_of(cap[i]) * sizeof(RecombItem);
    });
    auto chunk_sum = [&](const std::vector<uint64_t> *a, bool tiles) {
        return max_over(chunks, [&](const WinChunk &c) {
            uint64_t sum = 0;
            for (uint64_t i = c.w_begin; i < c.w_end; ++i) sum += a ? (*a)[i] : tiles ? tiles_of(cap[i]) : cap[i];
            return sum;
        });
    };
    const size_t max_wins = max_over(chunks, [](const WinChunk &c) { return c.w_end - c.w_begin; }), max_blocks = chunk_sum(&nb, false),
                 max_slots = chunk_sum(nullptr, false), max_items = std::max<size_t>(chunk_sum(nullptr, true), 1);
    REQUIRE(max_wins < 0x7FFFFFFFull && max_items < 0x7FFFFFFFull, "%s: a chunk of %zu windows exceeds one launch", fn, max_wins);

    // device: P as dwords | windows, items (up, through the page-locked staging with the same offsets) | records (down, staged) |
    // (q, m) per window | qualifying masks | gathered rows, their c, their coordinates, the site list, the site table
    Carve L;
    const size_t o_pbits = L.take<uint32_t>(wps), o_wins = L.take<LdWin>(max_wins), o_items = L.take<RecombItem>(max_items),
                 o_rec = L.take<impop_recomb_stats>(max_wins), staged = L.total(), o_qm = L.take<uint32_t>(2 * max_wins),
                 o_qmask = L.take<uint64_t>(max_blocks), o_rows = L.take<uint32_t>(max_slots * wps), o_cs = L.take<uint32_t>(max_slots),
                 o_coords = L.take<uint64_t>(max_slots), o_list = L.take<uint64_t>(max_slots),
                 o_tab = L.take<impop_recomb_site>(max_slots);
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

    const uint32_t WR = wps <= 4 ? 4u : wps <= 8 ? 8u : wps <= 16 ? 16u : wps <= 32 ? 32u : 0u;
    const size_t lds_pairs = ((size_t)RC_T * (WR ? WR : wps) + RC_T) * 4;

    const uint32_t *d_pbits = (const uint32_t *)(dc + o_pbits);
    const LdWin *d_wins = (const LdWin *)(dc + o_wins);
    const RecombItem *d_items = (const RecombItem *)(dc + o_items);
    impop_recomb_stats *d_rec = (impop_recomb_stats *)(dc + o_rec);
    uint32_t *d_qm = (uint32_t *)(dc + o_qm), *d_rows = (uint32_t *)(dc + o_rows), *d_cs = (uint32_t *)(dc + o_cs);
    uint64_t *d_qmask = (uint64_t *)(dc + o_qmask), *d_coords = (uint64_t *)(dc + o_coords), *d_list = (uint64_t *)(dc + o_list);
    impop_recomb_site *d_tab = (impop_recomb_site *)(dc + o_tab);
    LdWin *h_wins = (LdWin *)(hc + o_wins);
    RecombItem *h_items = (RecombItem *)(hc + o_items);
    std::vector<uint64_t> h_coords(used_sites ? max_slots : 0);
    std::vector<impop_recomb_site> h_tab(site_table ? max_slots : 0);
    EventPairs *timer = ctx->timers + impop_ctx::T_RECOMB;
    uint64_t launches = 0, qualifying = 0, used = 0, pair_tiles = 0;
    for (const WinChunk &c : chunks) {
        const size_t cnt = c.w_end - c.w_begin;
        uint64_t n_blocks = 0, longest = 0, n_slots = 0;  // blocks of all the chunk's windows / of its longest one; its slots
        uint32_t n_items = 0;
        for (size_t k = 0; k < cnt; ++k) {
            const uint64_t i = c.w_begin + k;
            h_wins[k] = LdWin{mapped[i].site_begin, mapped[i].site_end, n_blocks, n_slots,
                              (uint32_t)window_W(m, windows[i].site_begin, windows[i].site_end), cap[i]};
            n_blocks += nb[i];
            longest = std::max(longest, nb[i]);
            n_slots += cap[i];
            for (uint32_t t = 0; t < tiles_of(cap[i]); ++t) h_items[n_items++] = RecombItem{(uint32_t)k, t};
        }
        if (!n_items) h_items[n_items++] = RecombItem{0u, 0u};  // windows without sites only: the one item finds m = 0 and leaves
        if ((rc = run.up(o_wins, o_items + n_items * sizeof(RecombItem)))) return rc;
        if ((rc = run.timed(timer[0], [&] {
            hipLaunchKernelGGL(ld_select_kernel, dim3((uint32_t)cnt, ld_select_slices(longest)), dim3(LD_T), 0, ctx->stream, m->d_sb, d_wins, wps,
                               m->g.G, m->g.r, d_pbits, nP, params->min_mac, d_qmask);
        }))) return rc;
        if ((rc = run.timed(timer[1], [&] {
            hipLaunchKernelGGL(ld_gather_kernel, dim3((uint32_t)cnt), dim3(LD_T), 0, ctx->stream, m->d_sb, d_wins, wps, m->g.G, m->g.r, d_pbits,
                               m->compact ? m->d_pos : nullptr, max_sites, d_qmask, d_rows, d_cs, d_coords, d_qm,
                               max_sites > LD_GATHER_LDS_SITES ? d_list : nullptr, ctx->d_err, DEV_ERR_RECOMB);
        }))) return rc;
        if ((rc = run.timed(timer[2], [&] {
            switch (WR) {
            case 4: return launch_recomb_pairs<4>(ctx, n_items, lds_pairs, d_rows, d_cs, d_qm, d_wins, d_items, wps, nP, d_tab);
            case 8: return launch_recomb_pairs<8>(ctx, n_items, lds_pairs, d_rows, d_cs, d_qm, d_wins, d_items, wps, nP, d_tab);
            case 16: return launch_recomb_pairs<16>(ctx, n_items, lds_pairs, d_rows, d_cs, d_qm, d_wins, d_items, wps, nP, d_tab);
            case 32: return launch_recomb_pairs<32>(ctx, n_items, lds_pairs, d_rows, d_cs, d_qm, d_wins, d_items, wps, nP, d_tab);
            default: return launch_recomb_pairs<0>(ctx, n_items, lds_pairs, d_rows, d_cs, d_qm, d_wins, d_items, wps, nP, d_tab);
            }
        }))) return rc;
        if ((rc = run.timed(timer[3], [&] {
            hipLaunchKernelGGL(recomb_finish_kernel, dim3((uint32_t)cnt), dim3(64), 0, ctx->stream, d_tab, d_coords, d_qm, d_wins, nP, d_rec,
                               ctx->d_err);
        }))) return rc;
        launches += 4;
        if (used_sites && n_slots) HIP_TRY(hipMemcpyAsync(h_coords.data(), d_coords, n_slots * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (site_table && n_slots)
            HIP_TRY(hipMemcpyAsync(h_tab.data(), d_tab, n_slots * sizeof(impop_recomb_site), hipMemcpyDeviceToHost, ctx->stream));
        if ((rc = run.finish(o_rec, o_rec + cnt * sizeof(impop_recomb_stats)))) return rc;
        const impop_recomb_stats *rv = (const impop_recomb_stats *)(hc + o_rec);
        for (size_t k = 0; k < cnt; ++k) {
            const uint64_t i = c.w_begin + k;
            impop_recomb_stats r = rv[k];
            REQUIRE(r.n_used <= cap[i], "%s: window %llu reports %u used sites in %u slots", fn, (unsigned long long)i, r.n_used, cap[i]);
            recomb_doubles(r);
            out_host[i] = r;
            qualifying += r.n_qualifying;
            used += r.n_used;
            pair_tiles += tiles_of(r.n_used);
            // the rows of the optional tables: n_used entries from the chunk's slots, zeros behind them
            if (used_sites) {
                memset(used_sites + i * max_sites, 0, (size_t)max_sites * 8);
                memcpy(used_sites + i * max_sites, h_coords.data() + h_wins[k].row_off, (size_t)r.n_used * 8);
            }
            if (site_table) {
                memset(site_table + i * max_sites, 0, (size_t)max_sites * sizeof(impop_recomb_site));
                memcpy(site_table + i * max_sites, h_tab.data() + h_wins[k].row_off, (size_t)r.n_used * sizeof(impop_recomb_site));
            }
        }
    }
    if (trace_on()) {
        fprintf(stderr, "[impop_recomb_scan] route=%s windows=%llu chunks=%llu launches=%llu qualifying=%llu used=%llu pair_tiles=%llu "
                "bytes_streamed=%llu\n", m->compact ? "compact" : "dense", (unsigned long long)n_windows, (unsigned long long)chunks.size(),
                (unsigned long long)launches, (unsigned long long)qualifying, (unsigned long long)used, (unsigned long long)pair_tiles,
                (unsigned long long)(bytes_streamed + used * 4ull * wps));
        fflush(stderr);
    }
    return IMPOP_OK;
}

IMPOP_API int impop_ctx_recomb_elapsed(impop_ctx *ctx, double kernel_ms[4], uint64_t *chunks) {
    REQUIRE(ctx && kernel_ms, "impop_ctx_recomb_elapsed: NULL argument");
    return ctx_timers_elapsed(ctx, impop_ctx::T_RECOMB, 4, 3, kernel_ms, chunks);
}
