// ibs.hip — impop_ibs_scan: pairwise identity-by-state tracts over a whole range of sites (include/impop_hip.h).
//
// The operand is the word-major transposed stream of ehh.hip, [64-site block][row] uint64, rows = the haplotypes that are in a
// pair, made per chunk of blocks from d_sb (a compacted matrix: from its kept sites, with d_pos for their coordinates; the
// variable-site index keeps no kept -> original table and is not used).  The range's edges are masked off in the transpose, so
// a walk sees no difference outside the range and the range's own edges close the outer tracts (dip_runs.h: dip_close).
//
// A workgroup owns a tile of 256 pairs (ibs_plan.h) and a sub-segment of the chunk's blocks, one pair per lane.  All-pairs
// form: a tile is 16 rows x 16 rows; the 32 rows' words of a batch of blocks are staged in LDS once (one 256-byte bank row per
// block: conflict-free ds_read_b64 whatever the lane pattern) and every lane XORs its two.  List form: the lanes read their two
// rows from the chunk's words directly.  Differences are found with ctz and appended to the pair's DipSummary.
//   sweep 1 (count), per chunk:  transpose -> walk<count>: a summary per (sub-segment, pair) -> combine: the pair's carried
//                                summary joined with the sub-segments' in order.  Behind the last chunk the close kernel writes
//                                the pair records (and checks run lengths + differences = the range's length).
//   offsets:                     host prefix over n_tracts (ibs_offsets); pair ranges whose segments fit the staging
//   sweep 2 (fill), per pair range and chunk (only when the list fits the caller's capacity, or windows are given):
//                                transpose -> walk<count> -> combine, which now leaves in every (sub-segment, pair) slot the join
//                                of everything LEFT of the sub-segment -> walk<fill>: every difference closes the tract in front
//                                of it and knows its slot (ibs_closed_before + the lane's running count); the tract is written
//                                at the pair's offset and added to the window tables.  The close kernel adds the last tract.
// A slot at or past the pair's announced n_tracts is never written: it sets the device error word instead.  Every loop is
// bounded by a count from the host or from sweep 1; no spin waits, no flags between workgroups.
#include <string.h>

#include <algorithm>
#include <vector>

#include "chunk_run.h"
#include "device_utils.h"
#include "dip_runs.h"
#include "ibs_plan.h"
#include "ibs_sweeps.h"
#include "ibs_transpose.h"
#include "internal.h"
#include "scan_route.h"
#include "win_chunks.h"

namespace impop {

static_assert(sizeof(DipSummary) == 40, "summaries are stored as 40-byte records");
constexpr int IBS_T = 256;
static_assert(IBS_T == (int)IBS_PAIRS, "one pair per lane");

// ibs_transpose_kernel: ibs_transpose.h

struct IbsArgs {
    const uint64_t *wm;    // the chunk's words
    const uint64_t *pos;   // compacted: the kept sites' original coordinates, else null
    const IbsTile *tiles;
    const uint32_t *rows;  // row -> haplotype
    const uint32_t *plist; // list form: the pairs' rows, in the caller's (h1, h2) order
    DipSummary *sum, *carry;
    impop_ibs_pair *rec;
    const uint64_t *off;   // fill, with a segment list: the pairs' offsets
    impop_ibs_segment *seg;  // the staging of pairs [p0, p1), or null
    uint32_t *err;
    IbsWindowsDev win;     // acc null: no windows
    uint64_t n_pairs, p0, p1, off0;
    uint64_t b, e;         // the range, original coordinates
    uint64_t blk_abs0, len, seg_blocks;  // the chunk: its first block in the matrix, its blocks, blocks per sub-segment
    uint32_t stride, n, min_sites, n_sub;
};

// a reported tract [s, t) of `pair`, the k-th of the pair
__device__ inline void ibs_emit(const IbsArgs &A, uint64_t pair, uint32_t h1, uint32_t h2, uint64_t s, uint64_t t, uint32_t k,
                                uint32_t announced) {
    if (k >= announced) {  // the counting sweep did not announce it: nothing is written
        atomicOr(A.err, DEV_ERR_IBS);
        return;
    }
    if (A.seg) {
        impop_ibs_segment o;
        o.h1 = h1;
        o.h2 = h2;
        o.begin = s;
        o.end = t;
        o.pair = (uint32_t)pair;
        o.flags = (s == A.b ? IMPOP_IBS_OPEN_LEFT : 0u) | (t == A.e ? IMPOP_IBS_OPEN_RIGHT : 0u);
        A.seg[A.off[pair] - A.off0 + k] = o;
    }
    if (A.win.acc) ibs_add_tract(A.win, s, t, [](unsigned long long *p, unsigned long long v) { atomicAdd(p, v); });
}

// grid = (tiles, sub-segments of the chunk).  FILL: sum holds the join of everything left of each (sub-segment, pair).
template <bool ALL, bool FILL>
__global__ __launch_bounds__(IBS_T) void ibs_walk_kernel(const IbsArgs A) {
    __shared__ uint64_t s_w[ALL ? IBS_BATCH * 2 * IBS_TILE : 1];
    const uint32_t tid = threadIdx.x;
    const IbsTile tile = A.tiles[blockIdx.x];
    const uint32_t sub = blockIdx.y;
    uint32_t r1, r2;
    uint64_t pair;
    bool on;
    if (ALL) {
        r1 = tile.a0 * IBS_TILE + (tid >> 4);
        r2 = tile.b0 * IBS_TILE + (tid & 15);
        on = r1 < r2 && r2 < A.n;
        pair = on ? ibs_pair_index(A.n, r1, r2) : 0;
    } else {
        pair = (uint64_t)tile.a0 * IBS_PAIRS + tid;
        on = pair < A.n_pairs;
        r1 = on ? A.plist[2 * pair] : 0;
        r2 = on ? A.plist[2 * pair + 1] : 0;
    }
    on = on && pair >= A.p0 && pair < A.p1;
    const uint64_t slot = (uint64_t)sub * A.n_pairs + pair;
    DipSummary s = dip_empty();
    uint32_t k = 0, announced = 0, h1 = 0, h2 = 0;
    if (FILL && on) {
        s = A.sum[slot];
        k = ibs_closed_before(s, A.b, A.min_sites);
        announced = A.rec[pair].n_tracts;
        h1 = A.rows[r1];
        h2 = A.rows[r2];
    }
    const uint64_t lb0 = (uint64_t)sub * A.seg_blocks, lb1 = lb0 + A.seg_blocks < A.len ? lb0 + A.seg_blocks : A.len;
    for (uint64_t batch = lb0; batch < lb1; batch += IBS_BATCH) {  // the same trip count for every lane: the barriers are workgroup-wide
        const uint32_t nb = lb1 - batch < (uint64_t)IBS_BATCH ? (uint32_t)(lb1 - batch) : IBS_BATCH;
        if (ALL) {
            for (uint32_t i = tid; i < nb * 2 * IBS_TILE; i += IBS_T) {
                const uint32_t blk = i >> 5, q = i & 31;
                const uint32_t row = q < IBS_TILE ? tile.a0 * IBS_TILE + q : tile.b0 * IBS_TILE + (q - IBS_TILE);
                s_w[i] = row < A.n ? A.wm[(batch + blk) * A.stride + row] : 0ull;
            }
            __syncthreads();
        }
        if (on) {
            for (uint32_t blk = 0; blk < nb; ++blk) {
                uint64_t x;
                if (ALL) x = s_w[blk * 32 + (tid >> 4)] ^ s_w[blk * 32 + IBS_TILE + (tid & 15)];
                else x = A.wm[(batch + blk) * A.stride + r1] ^ A.wm[(batch + blk) * A.stride + r2];
                const uint64_t base = (A.blk_abs0 + batch + blk) * 64;
                for (; x; x &= x - 1) {
                    const uint64_t col = base + (uint32_t)__builtin_ctzll(x);
                    const uint64_t p = A.pos ? A.pos[col] : col;
                    if (FILL) {
                        const uint64_t beg = s.het ? s.last + 1 : A.b;
                        if (p - beg >= A.min_sites) {  // min_sites >= 1
                            ibs_emit(A, pair, h1, h2, beg, p, k, announced);
                            ++k;
                        }
                    }
                    dip_append_site(s, p, A.min_sites);
                }
            }
        }
        if (ALL) __syncthreads();
    }
    if (!FILL && on) A.sum[slot] = s;
}

// a thread's pair in the per-pair kernels.  ALL: grid = (ceil(n / 256), n), blockIdx.y = the first row; list: grid = ceil(pairs / 256)
template <bool ALL>
__device__ inline bool ibs_my_pair(const IbsArgs &A, uint64_t &pair, uint32_t &r1, uint32_t &r2) {
    bool on;
    if (ALL) {
        r1 = blockIdx.y;
        r2 = blockIdx.x * IBS_T + threadIdx.x;
        on = r1 < r2 && r2 < A.n;
        pair = on ? ibs_pair_index(A.n, r1, r2) : 0;
    } else {
        pair = (uint64_t)blockIdx.x * IBS_T + threadIdx.x;
        on = pair < A.n_pairs;
        r1 = on ? A.plist[2 * pair] : 0;
        r2 = on ? A.plist[2 * pair + 1] : 0;
    }
    return on && pair >= A.p0 && pair < A.p1;
}

// carry = carry joined with the chunk's sub-segments in order; keep_left: every slot receives what lies left of it
template <bool ALL>
__global__ __launch_bounds__(IBS_T) void ibs_combine_kernel(const IbsArgs A, int keep_left) {
    uint64_t pair;
    uint32_t r1, r2;
    if (!ibs_my_pair<ALL>(A, pair, r1, r2)) return;
    DipSummary E = A.carry[pair];
    for (uint32_t kk = 0; kk < A.n_sub; ++kk) {
        const uint64_t slot = (uint64_t)kk * A.n_pairs + pair;
        const DipSummary t = A.sum[slot];
        if (keep_left) A.sum[slot] = E;
        E = dip_combine(E, t, A.min_sites);
    }
    A.carry[pair] = E;
}

// behind the last chunk.  fill == 0: the pair record; fill != 0: the tract behind the last difference, and the slot count
template <bool ALL>
__global__ __launch_bounds__(IBS_T) void ibs_close_kernel(const IbsArgs A, int fill) {
    uint64_t pair;
    uint32_t r1, r2;
    if (!ibs_my_pair<ALL>(A, pair, r1, r2)) return;
    const DipSummary s = A.carry[pair];
    const uint32_t h1 = A.rows[r1], h2 = A.rows[r2];
    if (!fill) {
        const DipSummary c = dip_close(s, A.b, A.e, A.min_sites);
        if ((uint64_t)c.run_sum + c.het != A.e - A.b) atomicOr(A.err, DEV_ERR_IBS);
        impop_ibs_pair o;
        o.h1 = h1;
        o.h2 = h2;
        o.n_diff = c.het;
        o.longest = c.longest;
        o.n_tracts = c.roh_runs;
        o.reserved = 0;
        o.tract_sites = c.roh_sites;
        A.rec[pair] = o;
        return;
    }
    const uint32_t announced = A.rec[pair].n_tracts;
    uint32_t k = ibs_closed_before(s, A.b, A.min_sites);
    const uint64_t beg = s.het ? s.last + 1 : A.b;
    if (A.e - beg >= A.min_sites) {
        ibs_emit(A, pair, h1, h2, beg, A.e, k, announced);
        ++k;
    }
    if (k != announced) atomicOr(A.err, DEV_ERR_IBS);
}

template <bool ALL>
static void ibs_launch_pairs(impop_ctx *ctx, const IbsArgs &A, int which, int flag) {
    const dim3 grid = ALL ? dim3((A.n + IBS_T - 1) / IBS_T, A.n) : dim3((uint32_t)((A.n_pairs + IBS_T - 1) / IBS_T));
    if (which == 0) hipLaunchKernelGGL(ibs_combine_kernel<ALL>, grid, dim3(IBS_T), 0, ctx->stream, A, flag);
    else hipLaunchKernelGGL(ibs_close_kernel<ALL>, grid, dim3(IBS_T), 0, ctx->stream, A, flag);
}
template <bool ALL>
static void ibs_launch_walk(impop_ctx *ctx, const IbsArgs &A, uint32_t n_tiles, bool fill) {
    const dim3 grid(n_tiles, A.n_sub);
    if (fill) hipLaunchKernelGGL((ibs_walk_kernel<ALL, true>), grid, dim3(IBS_T), 0, ctx->stream, A);
    else hipLaunchKernelGGL((ibs_walk_kernel<ALL, false>), grid, dim3(IBS_T), 0, ctx->stream, A);
}

}  // namespace impop

using namespace impop;

// The two sweeps of impop_ibs_scan for the range [b, e) (e == 0: the matrix's end).  client null: the call itself.  Else
// (impop_ibd_scan, ibs_sweeps.h) the tracts stay on the device: every pair range is filled into the staging and handed to the client.
int impop::ibs_scan_run(const char *fn, impop_ctx *ctx, const impop_matrix *m, const uint64_t *mask_p, const uint32_t *pairs, uint64_t n_pairs,
                        const impop_window *windows, uint64_t n_windows, uint64_t b, uint64_t e, uint32_t min_sites,
                        uint64_t max_chunk_bytes, impop_ibs_pair *pair_out, impop_ibs_segment *seg_out, uint64_t seg_capacity,
                        uint64_t *n_segments, impop_ibs_window *win_out, IbsClient *client) {
    REQUIRE(m->device == ctx->device, "%s: matrix lives on device %d, context on %d", fn, m->device, ctx->device);
    REQUIRE(min_sites >= 1, "%s: min_sites must be at least 1", fn);
    const uint64_t span = matrix_span(m);
    if (!e) e = span;
    REQUIRE(b < e && e <= span, "%s: bad range [%llu,%llu) for %llu sites", fn, (unsigned long long)b, (unsigned long long)e,
            (unsigned long long)span);
    REQUIRE(e - b < (1ull << 32), "%s: a range of %llu sites does not fit the records' 32-bit lengths", fn, (unsigned long long)(e - b));
    REQUIRE(!(pairs && mask_p), "%s: give either a pair list or a member mask", fn);
    REQUIRE((windows == nullptr) == (win_out == nullptr), "%s: windows and win_out must both be given or both be NULL", fn);
    const uint32_t nh = m->g.n_hap, wps = m->g.wps, n_pad = wps * 32;
    const bool all = pairs == nullptr;

    // the rows: the members, or the haplotypes of the list; the list's pairs as rows
    MemberSet R;
    std::vector<uint32_t> plist;
    if (all) {
        R = member_set(mask_p, nh, wps);
        REQUIRE(R.size() >= 2, "%s: %u members make no pair", fn, R.size());
        if (R.size() > IMPOP_IBS_MAX_N) {
            set_error("%s: %u members exceed the all-pairs limit (%u)", fn, R.size(), (uint32_t)IMPOP_IBS_MAX_N);
            return IMPOP_E_UNSUPPORTED;
        }
        n_pairs = (uint64_t)R.size() * (R.size() - 1) / 2;
    } else {
        REQUIRE(n_pairs > 0, "%s: no pairs", fn);
        if (n_pairs > IMPOP_IBS_MAX_PAIRS) {
            set_error("%s: %llu pairs exceed the limit (%u)", fn, (unsigned long long)n_pairs, (uint32_t)IMPOP_IBS_MAX_PAIRS);
            return IMPOP_E_UNSUPPORTED;
        }
        std::vector<uint64_t> used((nh + 63) / 64, 0ull);
        for (uint64_t i = 0; i < n_pairs; ++i) {
            const uint32_t h1 = pairs[2 * i], h2 = pairs[2 * i + 1];
            REQUIRE(h1 < nh && h2 < nh, "%s: pair %llu: haplotype index %u outside the matrix's %u", fn, (unsigned long long)i,
                    h1 < nh ? h2 : h1, nh);
            REQUIRE(h1 != h2, "%s: pair %llu: both rows are haplotype %u", fn, (unsigned long long)i, h1);
            used[h1 >> 6] |= 1ull << (h1 & 63);
            used[h2 >> 6] |= 1ull << (h2 & 63);
        }
        R = member_set(used.data(), nh, wps);
        plist.resize(2 * n_pairs);
        for (uint64_t i = 0; i < 2 * n_pairs; ++i) plist[i] = (uint32_t)R.ppos[pairs[i]];
    }
    for (uint64_t i = 0; i < (windows ? n_windows : 0); ++i)
        REQUIRE(b <= windows[i].site_begin && windows[i].site_begin <= windows[i].site_end && windows[i].site_end <= e,
                "%s: window %llu [%llu,%llu) is not inside the range [%llu,%llu)", fn, (unsigned long long)i,
                (unsigned long long)windows[i].site_begin, (unsigned long long)windows[i].site_end, (unsigned long long)b,
                (unsigned long long)e);
    const bool want_win = windows && n_windows > 0;
    const uint32_t n = R.size(), stride = n;

    // the range's columns of d_sb and their blocks
    const uint64_t cb = m->compact ? pos_lower_bound(m, b) : b, ce = m->compact ? pos_lower_bound(m, e) : e;
    const uint64_t blk0 = cb >> 6, n_blk = ce > cb ? ((ce + 63) >> 6) - blk0 : 0;
    const uint64_t budget = chunk_budget(max_chunk_bytes);
    const std::vector<IbsTile> tiles_all = all ? ibs_tiles_all(n, 0, n_pairs) : ibs_tiles_list(0, n_pairs);
    const IbsCut cut = ibs_cut(n_blk, stride, n_pairs, tiles_all.size(), (uint32_t)ctx->n_cu, budget / 2,
                               env_tile_blocks("IMPOP_IBS_CHUNK_BLOCKS"), env_tile_blocks("IMPOP_IBS_SEG_BLOCKS"));
    const uint64_t seg_cap = std::max<uint64_t>(1, (budget / 2) / sizeof(impop_ibs_segment));

    IbsWindowPlan wp;
    if (want_win) {
        std::vector<uint64_t> wb(n_windows), we(n_windows);
        for (uint64_t i = 0; i < n_windows; ++i) {
            wb[i] = windows[i].site_begin;
            we[i] = windows[i].site_end;
        }
        wp.build(wb.data(), we.data(), n_windows);
    }

    // device: ppos | pmask | rows | tiles | list | window tables | words | summaries | carry | records; offsets and the segment
    // staging follow once sweep 1 has told their size
    Carve L;
    const size_t o_ppos = L.take<int32_t>(n_pad), o_pmask = L.take<uint32_t>(wps), o_rows = L.take<uint32_t>(n),
                 o_tiles = L.take<IbsTile>(tiles_all.size()), o_plist = L.take<uint32_t>(plist.size()),
                 o_edge = L.take<uint64_t>(wp.edge.size()), o_sbeg = L.take<uint64_t>(wp.sbeg.size()),
                 o_send = L.take<uint64_t>(wp.send.size()), o_acc = L.take<unsigned long long>(want_win ? wp.acc_words() : 0),
                 o_wm = L.take<uint64_t>(cut.chunk_blocks * stride), o_sum = L.take<DipSummary>((uint64_t)cut.n_sub * n_pairs),
                 o_carry = L.take<DipSummary>(n_pairs), o_rec = L.take<impop_ibs_pair>(n_pairs),
                 o_extra = L.take_bytes(client ? client->extra_bytes : 0), fixed = L.total();
    HIP_TRY(hipSetDevice(ctx->device));
    void *d = nullptr;
    int rc = ctx_scratch(ctx, fixed, &d);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemcpyAsync(L.at<char>(d, o_ppos), R.ppos.data(), (size_t)n_pad * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(L.at<char>(d, o_pmask), R.bits.data(), (size_t)wps * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(L.at<char>(d, o_rows), R.idx.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    if (!all) HIP_TRY(hipMemcpyAsync(L.at<char>(d, o_plist), plist.data(), plist.size() * 4, hipMemcpyHostToDevice, st));
    if (want_win) {
        HIP_TRY(hipMemcpyAsync(L.at<char>(d, o_edge), wp.edge.data(), wp.edge.size() * 8, hipMemcpyHostToDevice, st));
        if (!wp.sbeg.empty()) {
            HIP_TRY(hipMemcpyAsync(L.at<char>(d, o_sbeg), wp.sbeg.data(), wp.sbeg.size() * 8, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(L.at<char>(d, o_send), wp.send.data(), wp.send.size() * 8, hipMemcpyHostToDevice, st));
        }
        HIP_TRY(hipMemsetAsync(L.at<char>(d, o_acc), 0, wp.acc_words() * 8, st));
    }

    IbsArgs A{};
    A.wm = L.at<uint64_t>(d, o_wm);
    A.pos = m->compact ? m->d_pos : nullptr;
    A.tiles = L.at<IbsTile>(d, o_tiles);
    A.rows = L.at<uint32_t>(d, o_rows);
    A.plist = all ? nullptr : L.at<uint32_t>(d, o_plist);
    A.sum = L.at<DipSummary>(d, o_sum);
    A.carry = L.at<DipSummary>(d, o_carry);
    A.rec = L.at<impop_ibs_pair>(d, o_rec);
    A.err = ctx->d_err;
    A.n_pairs = n_pairs;
    A.b = b;
    A.e = e;
    A.seg_blocks = cut.seg_blocks;
    A.stride = stride;
    A.n = n;
    A.min_sites = min_sites;

    if (client && client->prepare && (rc = client->prepare(L.at<char>(d, o_extra), n_pairs))) return rc;
    EventPairs *timer = ctx->timers + (client ? client->timer : (int)impop_ctx::T_IBS);
    uint64_t launches = 0, bytes_streamed = 0, chunks_run = 0, subs_run = 0;
    std::vector<IbsTile> tiles;  // of the sweep in flight: alive until its synchronisation
    // one sweep over the range's chunks for the pairs [p0, p1); A.seg / A.off / A.win say what a fill leaves behind
    auto sweep = [&](bool fill, uint64_t p0, uint64_t p1) -> int {
        int rc2;
        A.p0 = p0;
        A.p1 = p1;
        tiles = (p0 == 0 && p1 == n_pairs) ? tiles_all : all ? ibs_tiles_all(n, p0, p1) : ibs_tiles_list(p0, p1);
        const uint32_t nt = (uint32_t)tiles.size();
        HIP_TRY(hipMemcpyAsync(L.at<char>(d, o_tiles), tiles.data(), (size_t)nt * sizeof(IbsTile), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(A.carry, 0, n_pairs * sizeof(DipSummary), st));  // dip_empty() is all zeros
        for (uint64_t c = 0; c < cut.n_chunks; ++c) {
            A.len = cut.chunk_len(c, n_blk);
            A.blk_abs0 = blk0 + cut.chunk_begin(c);
            A.n_sub = cut.subs_of(A.len);
            if ((rc2 = timed(ctx, timer[0], [&] {
                hipLaunchKernelGGL(ibs_transpose_kernel, dim3((uint32_t)((A.len + 3) / 4)), dim3(256), 0, st, m->d_sb, wps, m->g.G, m->g.r,
                                   L.at<int32_t>(d, o_ppos), L.at<uint32_t>(d, o_pmask), A.blk_abs0, A.len, cb, ce, stride,
                                   L.at<uint64_t>(d, o_wm));
            }))) return rc2;
            if ((rc2 = timed(ctx, timer[1], [&] { all ? ibs_launch_walk<true>(ctx, A, nt, false) : ibs_launch_walk<false>(ctx, A, nt, false); })))
                return rc2;
            if ((rc2 = timed(ctx, timer[2], [&] { all ? ibs_launch_pairs<true>(ctx, A, 0, fill) : ibs_launch_pairs<false>(ctx, A, 0, fill); })))
                return rc2;
            launches += 3;
            if (fill) {
                if ((rc2 = timed(ctx, timer[1], [&] { all ? ibs_launch_walk<true>(ctx, A, nt, true) : ibs_launch_walk<false>(ctx, A, nt, true); })))
                    return rc2;
                ++launches;
            }
            const uint64_t walk_bytes = all ? (uint64_t)nt * A.len * 2 * IBS_TILE * 8 : (p1 - p0) * A.len * 16;
            bytes_streamed += A.len * 64 * wps * 4 + walk_bytes * (fill ? 2 : 1);
            ++chunks_run;
            subs_run += A.n_sub;
        }
        if ((rc2 = timed(ctx, timer[2], [&] { all ? ibs_launch_pairs<true>(ctx, A, 1, fill) : ibs_launch_pairs<false>(ctx, A, 1, fill); })))
            return rc2;
        ++launches;
        return IMPOP_OK;
    };
    auto sync_checked = [&]() -> int {
        const int rc2 = ctx_err_fetch(ctx);
        if (rc2) return rc2;
        HIP_TRY(hipStreamSynchronize(st));
        return ctx_err_result(ctx, fn);
    };

    // sweep 1: the pair records
    if ((rc = sweep(false, 0, n_pairs))) return rc;
    std::vector<impop_ibs_pair> rec_host;
    impop_ibs_pair *recs = pair_out;
    if (!recs) {
        rec_host.resize(n_pairs);
        recs = rec_host.data();
    }
    HIP_TRY(hipMemcpyAsync(recs, A.rec, n_pairs * sizeof(impop_ibs_pair), hipMemcpyDeviceToHost, st));
    if ((rc = sync_checked())) return rc;
    const std::vector<uint64_t> off = ibs_offsets(n_pairs, [&](uint64_t p) { return recs[p].n_tracts; });
    const uint64_t total = off[n_pairs];
    *n_segments = total;

    // sweep 2: the segment list, where it fits, and the window tables
    // a client's tracts always go through the staging, and it sees every pair range, tracts or none
    const bool want_seg = client || (seg_out && seg_capacity >= total && total > 0);
    uint64_t ranges_run = 0;
    if (want_seg || (want_win && total > 0)) {
        const std::vector<uint64_t> ranges = want_seg ? ibs_pair_ranges(off, seg_cap) : std::vector<uint64_t>{0, n_pairs};
        uint64_t max_seg = 0;
        for (size_t k = 0; want_seg && k + 1 < ranges.size(); ++k) max_seg = std::max(max_seg, off[ranges[k + 1]] - off[ranges[k]]);
        // offsets | segment staging: a side buffer of their own, so that the scratch of sweep 1 stays where it is
        Carve L2;
        const size_t o_off = L2.take<uint64_t>(want_seg ? n_pairs + 1 : 0), o_seg = L2.take<impop_ibs_segment>(max_seg);
        void *d2 = nullptr;
        if ((rc = ctx_aux(ctx, 0, L2.total() + 256, &d2))) return rc;
        if (want_seg) {
            HIP_TRY(hipMemcpyAsync(L2.at<char>(d2, o_off), off.data(), (n_pairs + 1) * 8, hipMemcpyHostToDevice, st));
            A.off = L2.at<uint64_t>(d2, o_off);
        }
        if (want_win) {
            A.win.edge = L.at<uint64_t>(d, o_edge);
            A.win.sbeg = L.at<uint64_t>(d, o_sbeg);
            A.win.send = L.at<uint64_t>(d, o_send);
            A.win.acc = L.at<unsigned long long>(d, o_acc);
            A.win.n_edge = (uint32_t)wp.edge.size();
            A.win.n_span = (uint32_t)wp.sbeg.size();
        }
        for (size_t k = 0; k + 1 < ranges.size(); ++k) {
            const uint64_t p0 = ranges[k], p1 = ranges[k + 1], cnt = off[p1] - off[p0];
            if (cnt == 0 && !want_win && !client) continue;
            A.seg = want_seg ? L2.at<impop_ibs_segment>(d2, o_seg) : nullptr;
            A.off0 = off[p0];
            ++ranges_run;
            if (client) {
                if (cnt && (rc = sweep(true, p0, p1))) return rc;
                if ((rc = client->range(IbsStage{p0, p1, n_pairs, A.rec, A.off, A.seg, off[p0], cnt}))) return rc;  // synchronises
                continue;
            }
            if ((rc = sweep(true, p0, p1))) return rc;
            if (want_seg && cnt)
                HIP_TRY(hipMemcpyAsync(seg_out + off[p0], A.seg, cnt * sizeof(impop_ibs_segment), hipMemcpyDeviceToHost, st));
            if ((rc = sync_checked())) return rc;
        }
    }
    if (want_win) {
        std::vector<unsigned long long> acc(wp.acc_words(), 0ull);
        if (total > 0) {
            HIP_TRY(hipMemcpyAsync(acc.data(), L.at<char>(d, o_acc), acc.size() * 8, hipMemcpyDeviceToHost, st));
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
            o.share = we > wb ? (double)o.pair_sites / ((double)n_pairs * (double)(we - wb)) : __builtin_nan("");
            win_out[i] = o;
        }
    }
    if (client) {
        client->n_pairs = n_pairs;
        client->tracts = total;
        client->pair_ranges = ranges_run;
        client->launches = launches;
        client->bytes_streamed = bytes_streamed;
        return IMPOP_OK;
    }
    if (trace_on()) {
        fprintf(stderr, "[impop_ibs_scan] route=%s pairs=%llu site_chunks=%llu sub_segments=%llu launches=%llu tracts=%llu bytes_streamed=%llu\n",
                m->compact ? "compact" : "dense", (unsigned long long)n_pairs, (unsigned long long)chunks_run, (unsigned long long)subs_run,
                (unsigned long long)launches, (unsigned long long)total, (unsigned long long)bytes_streamed);
        fflush(stderr);
    }
    return IMPOP_OK;
}

IMPOP_API int impop_ibs_scan(impop_ctx *ctx, const impop_matrix *m, const uint64_t *mask_p, const uint32_t *pairs, uint64_t n_pairs,
                             const impop_window *windows, uint64_t n_windows, const impop_ibs_params *params, impop_ibs_pair *pair_out,
                             impop_ibs_segment *seg_out, uint64_t seg_capacity, uint64_t *n_segments, impop_ibs_window *win_out) {
    static_assert(sizeof(impop_ibs_params) == 32 && sizeof(impop_ibs_pair) == 32 && sizeof(impop_ibs_segment) == 32 &&
                      sizeof(impop_ibs_window) == 32,
                  "ABI layout");
    REQUIRE(ctx && m && params && n_segments, "%s: NULL argument", "impop_ibs_scan");
    REQUIRE(params->struct_size == sizeof(impop_ibs_params), "impop_ibs_params.struct_size mismatch");
    return ibs_scan_run("impop_ibs_scan", ctx, m, mask_p, pairs, n_pairs, windows, n_windows, params->site_begin, params->site_end,
                        params->min_sites, params->max_chunk_bytes, pair_out, seg_out, seg_capacity, n_segments, win_out, nullptr);
}

IMPOP_API int impop_ctx_ibs_elapsed(impop_ctx *ctx, double kernel_ms[3], uint64_t *chunks) {
    REQUIRE(ctx && kernel_ms, "impop_ctx_ibs_elapsed: NULL argument");
    return ctx_timers_elapsed(ctx, impop_ctx::T_IBS, 3, 0, kernel_ms, chunks);
}
