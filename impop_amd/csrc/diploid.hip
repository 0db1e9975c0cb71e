// diploid.hip — impop_diploid_scan: the individual level of a windowed scan.  Two haplotypes of the matrix are the two copies of one
// diploid person; per window and per person: heterozygous sites, sites homozygous for the allele and the runs of homozygosity
// between heterozygous sites; per window: observed and expected heterozygosity, F_IS, F_ROH (include/impop_hip.h).
//
// Windows are mapped straight onto d_sb, which holds every row of the matrix whatever index was built beside it (a compacted
// matrix: onto its kept sites, with d_pos for their coordinates — the dropped sites are monomorphic, nobody is heterozygous
// there, and those that every haplotype carries are counted into hom_alt from the matrix's bitmap of them), so a record cannot
// depend on the upload's keep flags.  The variable-site index is not used: it keeps no kept-site -> original-coordinate table,
// and runs need coordinates.  Per chunk of windows, on the tiles of cut_tiles (elementary segments: a tile's interior is the
// same for every window that contains it, so overlapping windows share tiles), two launches:
//   1. dip_tile_kernel    one workgroup per tile.  Every wave takes a contiguous share of the tile's 64-site blocks, in block
//                         order.  Per block, lane = site: c = carriers among the 2N -> sum_p, s_p; the ballot transpose of every
//                         dword column that holds a member -> per-haplotype 64-site words in the wave's LDS; lane = individual:
//                         het = word(h1) ^ word(h2), hom_alt = word(h1) & word(h2), every heterozygous site appended to the
//                         individual's summary (dip_runs.h) of this wave.  The waves' summaries are then joined in wave order and
//                         stored with one plain store per individual.  No global atomics, no floating point.
//   2. dip_window_kernel  one workgroup per window: a thread per individual joins the window's tile summaries in tile order,
//                         closes the leading and trailing run against the window's edges, writes the individual's row and adds
//                         it to the window's integers in LDS.  het_total is taken from the tiles' own count and compared with
//                         the rows' sum; every row's run lengths + het must give the window's length: else the device error word.
// The doubles of a record are computed on the host from its integers, in one place.  Chunks: win_chunks.h / chunk_run.h.
#include <string.h>

#include <algorithm>
#include <vector>

#include "device_utils.h"
#include "dip_runs.h"
#include "hap_words.h"
#include "internal.h"
#include "sb64.h"
#include "scan_route.h"
#include "win_chunks.h"

namespace impop {

constexpr int DIP_T = 256;                     // threads of a workgroup (the tile kernel: fewer waves when N is large)
constexpr size_t DIP_LDS_BUDGET = 144 * 1024;  // dynamic LDS of the tile kernel: 56 N bytes per wave
static_assert(sizeof(DipSummary) == 40, "tile summaries are stored as 40-byte records");

struct DipTileTotals {  // what a tile adds to every window that contains it
    uint64_t sum_p, het_total;
    uint32_t s_p, het_sites;
};
struct DipWin {           // a window of a chunk
    uint64_t b, e;        // original site coordinates
    uint32_t t0, t1;      // its tiles (chunk-local)
    uint32_t n_sites, pad;  // W
};

__device__ __forceinline__ uint64_t wave_or_u64(uint64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v |= __shfl_xor(v, off, 64);
    return v;
}

// grid = tiles of the chunk, block = 64 x waves.  Dynamic LDS: summaries [wave][N] (40 B) | words [wave][2 N] (8 B).
// ppos[h] = 2 i (+ 1): haplotype h is the first (second) copy of individual i, -1: in no pair; pmask[k]: the members of dword
// column k.  pos: the kept sites' original coordinates (compacted matrix), else null.
__global__ __launch_bounds__(DIP_T) void dip_tile_kernel(const uint32_t *__restrict__ sb, const uint64_t *__restrict__ pos,
                                                         const ScanTile *__restrict__ tiles, uint32_t wps, uint32_t G, uint32_t r,
                                                         const int32_t *__restrict__ ppos, const uint32_t *__restrict__ pmask, uint32_t N,
                                                         uint32_t min_run, DipSummary *__restrict__ tile_sum,
                                                         DipTileTotals *__restrict__ tile_tot) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dip_lds[];
    __shared__ unsigned long long s_sum_p, s_het_total;
    __shared__ uint32_t s_sp, s_het_sites;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = (uint32_t)__builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t n_waves = blockDim.x >> 6;
    DipSummary *sums = reinterpret_cast<DipSummary *>(dip_lds);
    unsigned long long *words = reinterpret_cast<unsigned long long *>(sums + (size_t)n_waves * N) + (size_t)wave * 2 * N;
    DipSummary *mine = sums + (size_t)wave * N;
    for (uint32_t i = lane; i < N; i += 64) mine[i] = dip_empty();
    if (tid == 0) {
        s_sum_p = 0;
        s_het_total = 0;
        s_sp = 0;
        s_het_sites = 0;
    }
    __syncthreads();
    const ScanTile t = tiles[blockIdx.x];
    const TileBlocks tb = tile_blocks_of(t);
    const uint64_t b0 = tb.b0, b1 = tb.b1;
    const uint64_t per = (b1 - b0 + n_waves - 1) / n_waves;  // blocks per wave: wave w takes [b0 + w per, b0 + (w + 1) per)
    const uint32_t n2 = 2 * N;
    uint64_t sum_p = 0, het_total = 0;
    uint32_t sp = 0, het_sites = 0;
    for (uint64_t j = 0; j < per; ++j) {  // the same trip count for every wave: the barriers are workgroup-wide
        const uint64_t b = b0 + (uint64_t)wave * per + j;
        const bool on = b < b1;
        if (on) {
            const uint64_t edge = hap_edge(t, b);
            uint32_t c = 0;
            sb_for_each_dword<true>(sb + b * 64ull * wps, G, r, lane, [&](uint32_t k, uint32_t w) {
                const uint32_t pm = (uint32_t)__builtin_amdgcn_readfirstlane(pmask[k]);
                if (pm == 0u) return;
                c += __popc(w & pm);
                const uint64_t word = ballot_transpose32(w, lane) & edge;
                if (lane < 32) {
                    const int32_t pp = ppos[32 * k + lane];
                    if (pp >= 0) words[pp] = word;
                }
            });
            if ((edge >> lane) & 1ull) {
                sum_p += (uint64_t)c * (n2 - c);
                sp += c > 0 && c < n2;
            }
        }
        __syncthreads();
        if (on) {
            const uint64_t base = b * 64;
            uint64_t any = 0;
            for (uint32_t i = lane; i < N; i += 64) {
                const uint64_t w1 = words[2 * i], w2 = words[2 * i + 1];
                uint64_t het = w1 ^ w2;
                const uint64_t hom = w1 & w2;
                if ((het | hom) == 0ull) continue;
                any |= het;
                het_total += (uint32_t)__popcll(het);
                DipSummary s = mine[i];
                s.hom_alt += (uint32_t)__popcll(hom);
                for (; het; het &= het - 1) {
                    const uint64_t site = base + (uint32_t)__builtin_ctzll(het);
                    dip_append_site(s, pos ? pos[site] : site, min_run);
                }
                mine[i] = s;
            }
            het_sites += (uint32_t)__popcll(wave_or_u64(any));  // the same in every lane: lane 0 reports it
        }
        __syncthreads();
    }
    sum_p = wave_sum_u64(sum_p);
    het_total = wave_sum_u64(het_total);
    sp = wave_sum_u32(sp);
    if (lane == 0) {
        atomicAdd(&s_sum_p, (unsigned long long)sum_p);
        atomicAdd(&s_het_total, (unsigned long long)het_total);
        atomicAdd(&s_sp, sp);
        atomicAdd(&s_het_sites, het_sites);
    }
    __syncthreads();
    DipSummary *dst = tile_sum + (uint64_t)blockIdx.x * N;
    for (uint32_t i = tid; i < N; i += blockDim.x) {
        DipSummary s = sums[i];
        for (uint32_t w = 1; w < n_waves; ++w) s = dip_combine(s, sums[(size_t)w * N + i], min_run);
        dst[i] = s;
    }
    if (tid == 0) tile_tot[blockIdx.x] = DipTileTotals{s_sum_p, s_het_total, s_sp, s_het_sites};
}

// grid = windows of the chunk.  ones (compacted matrix, else null): the bitmap, in original coordinates, of the dropped sites every
// haplotype carries — each is a hom_alt site of every individual.
__global__ __launch_bounds__(DIP_T) void dip_window_kernel(const DipSummary *__restrict__ tile_sum, const DipTileTotals *__restrict__ tile_tot,
                                                           const DipWin *__restrict__ wins, const uint32_t *__restrict__ ones, uint32_t N,
                                                           uint32_t min_run,
                                                           impop_diploid_stats *__restrict__ rec, impop_diploid_ind *__restrict__ ind,
                                                           uint32_t *__restrict__ err) {
    __shared__ unsigned long long s_het, s_roh_sites, s_sum_p, s_tile_het;
    __shared__ uint32_t s_runs, s_longest, s_sp, s_het_sites, s_bad, s_ones;
    const uint32_t tid = threadIdx.x;
    const DipWin w = wins[blockIdx.x];
    if (tid == 0) {
        s_het = s_roh_sites = s_sum_p = s_tile_het = 0;
        s_runs = s_longest = s_sp = s_het_sites = s_bad = s_ones = 0;
    }
    __syncthreads();
    if (ones && w.e > w.b) {
        const uint64_t d0 = w.b >> 5, d1 = (w.e + 31) >> 5;
        uint32_t cnt = 0;
        for (uint64_t d = d0 + tid; d < d1; d += DIP_T) {
            uint32_t v = ones[d];
            if (d == d0) v &= 0xFFFFFFFFu << (w.b & 31);
            if (d == d1 - 1 && (w.e & 31)) v &= 0xFFFFFFFFu >> (32 - (w.e & 31));
            cnt += __popc(v);
        }
        if (cnt) atomicAdd(&s_ones, cnt);
    }
    __syncthreads();
    const uint32_t hom_add = s_ones;
    unsigned long long het = 0, roh_sites = 0;
    uint32_t runs = 0, longest = 0, bad = 0;
    for (uint32_t i = tid; i < N; i += DIP_T) {
        DipSummary s = dip_empty();
        for (uint32_t t = w.t0; t < w.t1; ++t) s = dip_combine(s, tile_sum[(uint64_t)t * N + i], min_run);
        s = dip_close(s, w.b, w.e, min_run);
        bad |= (uint64_t)s.run_sum + s.het != w.e - w.b;
        if (ind) ind[(uint64_t)blockIdx.x * N + i] = impop_diploid_ind{s.het, s.hom_alt + hom_add, s.longest, s.roh_runs, s.roh_sites, 0u};
        het += s.het;
        roh_sites += s.roh_sites;
        runs += s.roh_runs;
        longest = longest > s.longest ? longest : s.longest;
    }
    unsigned long long sum_p = 0, tile_het = 0;
    uint32_t sp = 0, het_sites = 0;
    for (uint32_t t = w.t0 + tid; t < w.t1; t += DIP_T) {
        const DipTileTotals x = tile_tot[t];
        sum_p += x.sum_p;
        tile_het += x.het_total;
        sp += x.s_p;
        het_sites += x.het_sites;
    }
    if (het) atomicAdd(&s_het, het);
    if (roh_sites) atomicAdd(&s_roh_sites, roh_sites);
    if (runs) atomicAdd(&s_runs, runs);
    if (longest) atomicMax(&s_longest, longest);
    if (bad) atomicOr(&s_bad, 1u);
    if (sum_p) atomicAdd(&s_sum_p, sum_p);
    if (tile_het) atomicAdd(&s_tile_het, tile_het);
    if (sp) atomicAdd(&s_sp, sp);
    if (het_sites) atomicAdd(&s_het_sites, het_sites);
    __syncthreads();
    if (tid != 0) return;
    impop_diploid_stats o;
    o.n_ind = N;
    o.n_sites = w.n_sites;
    o.s_p = s_sp;
    o.het_sites = s_het_sites;
    o.het_total = s_tile_het;
    o.sum_p = s_sum_p;
    o.roh_sites_total = s_roh_sites;
    o.roh_runs_total = s_runs;
    o.longest_run = s_longest;
    o.ho = o.he = o.f_is = o.f_roh = 0.0;  // the host fills them in from the integers
    rec[blockIdx.x] = o;
    if (s_bad || s_tile_het != s_het) atomicOr(err, DEV_ERR_DIPLOID);
}

// The tile of scan.hip's streaming kernels (tile_cut.h, default_tile_rule).  IMPOP_DIPLOID_TILE_BLOCKS=n (1..4096) overrides it,
// so that tests reach many-tile windows on small matrices.
static uint32_t dip_tile_blocks(const impop_ctx *ctx, const impop_matrix *m, const std::vector<LayoutWindow> &lw) {
    if (const uint32_t e = env_tile_blocks("IMPOP_DIPLOID_TILE_BLOCKS")) return e;
    uint64_t blocks = 0;
    for (const LayoutWindow &w : lw) blocks += (w.hi.c - w.lo.c + 63) / 64;
    return default_tile_rule(m->g.wps, std::min<uint64_t>(blocks, m->g.n_block), ctx->n_cu);
}

}  // namespace impop

using namespace impop;

IMPOP_API int impop_diploid_scan(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows,
                                 const uint32_t *pairs, uint32_t n_ind, const impop_diploid_params *params, impop_diploid_stats *out_host,
                                 impop_diploid_ind *ind_out) {
    static_assert(sizeof(impop_diploid_stats) == 80 && sizeof(impop_diploid_ind) == 24 && sizeof(impop_diploid_params) == 16 &&
                      sizeof(DipWin) == 32 && sizeof(DipTileTotals) == 24,
                  "ABI layout");
    const char *fn = "impop_diploid_scan";
    REQUIRE(ctx && m && params, "%s: NULL argument", fn);
    REQUIRE(params->struct_size == sizeof(impop_diploid_params), "impop_diploid_params.struct_size mismatch");
    REQUIRE(m->device == ctx->device, "%s: matrix lives on device %d, context on %d", fn, m->device, ctx->device);
    REQUIRE(n_ind > 0 && pairs, "%s: no individuals", fn);
    REQUIRE(params->min_run >= 1, "%s: min_run must be at least 1", fn);
    if (n_ind > IMPOP_DIPLOID_MAX_N) {
        set_error("%s: %u individuals exceed the limit (%u)", fn, n_ind, (uint32_t)IMPOP_DIPLOID_MAX_N);
        return IMPOP_E_UNSUPPORTED;
    }
    const uint32_t n = m->g.n_hap, wps = m->g.wps, n_pad = wps * 32, N = n_ind, min_run = params->min_run;
    std::vector<int32_t> ppos(n_pad, -1);
    std::vector<uint32_t> pmask(wps, 0u);
    for (uint32_t i = 0; i < N; ++i) {
        const uint32_t h1 = pairs[2 * i], h2 = pairs[2 * i + 1];
        REQUIRE(h1 < n && h2 < n, "%s: individual %u: haplotype index %u outside the matrix's %u", fn, i, h1 < n ? h2 : h1, n);
        REQUIRE(h1 != h2, "%s: individual %u: both copies are haplotype %u", fn, i, h1);
        REQUIRE(ppos[h1] < 0 && ppos[h2] < 0, "%s: individual %u: haplotype %u is in two pairs", fn, i, ppos[h1] < 0 ? h2 : h1);
        ppos[h1] = (int32_t)(2 * i);
        ppos[h2] = (int32_t)(2 * i + 1);
        pmask[h1 >> 5] |= 1u << (h1 & 31);
        pmask[h2 >> 5] |= 1u << (h2 & 31);
    }
    int rc = check_windows(fn, m, windows, windows ? n_windows : 0);
    if (rc) return rc;
    if (!n_windows) return IMPOP_OK;
    REQUIRE(windows && out_host, "%s: NULL windows/out", fn);
    if ((rc = check_window_weights(fn, m, windows, n_windows))) return rc;

    // the rows of the matrix itself, whatever index was built beside them
    ScanRoute rt;
    rt.sb = m->d_sb;
    rt.lw = row_windows(m, windows, n_windows);
    rt.tile_blocks = dip_tile_blocks(ctx, m, rt.lw);
    cut_tiles(rt.lw, rt.tile_blocks, wps, false, rt);

    // device bytes of a chunk: per tile N summaries, the totals and the tile; per window the record, the descriptor and (if
    // wanted) N rows
    const TileCosts costs{(uint64_t)N * sizeof(DipSummary) + sizeof(DipTileTotals) + sizeof(ScanTile),
                          sizeof(impop_diploid_stats) + sizeof(DipWin) + (ind_out ? (uint64_t)N * sizeof(impop_diploid_ind) : 0), 0};
    const std::vector<TiledChunk> chunks =
        plan_tiled_chunks(rt.wins.data(), n_windows, rt.tiles.size(), chunk_budget(params->max_chunk_bytes), 0, costs);
    const size_t max_tiles = max_over(chunks, [](const TiledChunk &c) { return c.tiles.size(); }),
                 max_wins = max_over(chunks, [](const TiledChunk &c) { return c.w_end - c.w_begin; });
    REQUIRE(max_tiles < 0x7FFFFFFFull && max_wins < 0x7FFFFFFFull, "%s: a chunk of %zu tiles / %zu windows exceeds one launch", fn, max_tiles,
            max_wins);
    REQUIRE((uint64_t)max_tiles * N * sizeof(DipSummary) <= (64ull << 30), "%s: a window needs %llu MiB of tile summaries", fn,
            (unsigned long long)(((uint64_t)max_tiles * N * sizeof(DipSummary)) >> 20));

    // device: ppos | pmask | tiles | windows (up, through the page-locked staging with the same offsets) | records (down, staged) |
    // tile summaries | tile totals | rows
    Carve L;
    const size_t o_ppos = L.take<int32_t>(n_pad), o_pmask = L.take<uint32_t>(wps), o_fixed = L.total(), o_tiles = L.take<ScanTile>(max_tiles),
                 o_wins = L.take<DipWin>(max_wins), o_rec = L.take<impop_diploid_stats>(max_wins), staged = L.total(),
                 o_sum = L.take<DipSummary>(max_tiles * N), o_tot = L.take<DipTileTotals>(max_tiles),
                 o_ind = L.take<impop_diploid_ind>(ind_out ? max_wins * N : 0);
    HIP_TRY(hipSetDevice(ctx->device));
    void *d = nullptr, *pin = nullptr;
    rc = ctx_scratch(ctx, L.total(), &d);
    if (rc) return rc;
    rc = ctx_pinned(ctx, staged, &pin);
    if (rc) return rc;
    const ChunkRun run{ctx, fn, (char *)d, (char *)pin};
    char *dc = run.dc, *hc = run.hc;
    memcpy(hc + o_ppos, ppos.data(), (size_t)n_pad * 4);
    memcpy(hc + o_pmask, pmask.data(), (size_t)wps * 4);
    if ((rc = run.up(0, o_fixed))) return rc;

    // waves of a tile workgroup: as many of 4 as the LDS holds summaries and words for (N <= 658: 4, N = 2048: 1)
    const size_t lds_wave = (size_t)N * (sizeof(DipSummary) + 16);
    const uint32_t n_waves = (uint32_t)std::max<size_t>(1, std::min<size_t>(DIP_T / 64, DIP_LDS_BUDGET / lds_wave));
    const size_t lds_tile = lds_wave * n_waves;
    if ((rc = lds_opt_in(dip_tile_kernel, lds_tile))) return rc;

    const int32_t *d_ppos = (const int32_t *)(dc + o_ppos);
    const uint32_t *d_pmask = (const uint32_t *)(dc + o_pmask);
    const ScanTile *d_tiles = (const ScanTile *)(dc + o_tiles);
    const DipWin *d_wins = (const DipWin *)(dc + o_wins);
    impop_diploid_stats *d_rec = (impop_diploid_stats *)(dc + o_rec);
    DipSummary *d_sum = (DipSummary *)(dc + o_sum);
    DipTileTotals *d_tot = (DipTileTotals *)(dc + o_tot);
    impop_diploid_ind *d_ind = ind_out ? (impop_diploid_ind *)(dc + o_ind) : nullptr;
    ScanTile *h_tiles = (ScanTile *)(hc + o_tiles);
    DipWin *h_wins = (DipWin *)(hc + o_wins);
    EventPairs *timer = ctx->timers + impop_ctx::T_DIP;
    uint64_t launches = 0, bytes_streamed = 0, tiles_run = 0;
    for (const TiledChunk &c : chunks) {
        const size_t nt = c.tiles.size(), cnt = c.w_end - c.w_begin;
        for (size_t k = 0; k < nt; ++k) {
            h_tiles[k] = rt.tiles[c.tiles[k]];
            bytes_streamed += tile_bytes_streamed(h_tiles[k], wps);  // tiles of cut_tiles without an index: never empty, no rare entries
        }
        for (size_t k = 0; k < cnt; ++k) {
            const impop_window &w = windows[c.w_begin + k];
            const uint32_t l0 = c.l0[k], tiles_k = (uint32_t)(rt.wins[c.w_begin + k].t1 - rt.wins[c.w_begin + k].t0);
            h_wins[k] = DipWin{w.site_begin, w.site_end, l0, l0 + tiles_k, (uint32_t)window_W(m, w.site_begin, w.site_end), 0u};
        }
        if ((rc = run.up(o_tiles, o_rec))) return rc;  // from the tiles to the end of the windows
        if (nt) {
            if ((rc = run.timed(timer[0], [&] {
                hipLaunchKernelGGL(dip_tile_kernel, dim3((uint32_t)nt), dim3(64 * n_waves), lds_tile, ctx->stream, m->d_sb,
                                   m->compact ? m->d_pos : nullptr, d_tiles, wps, m->g.G, m->g.r, d_ppos, d_pmask, N, min_run, d_sum, d_tot);
            }))) return rc;
            ++launches;
        }
        if ((rc = run.timed(timer[1], [&] {
            hipLaunchKernelGGL(dip_window_kernel, dim3((uint32_t)cnt), dim3(DIP_T), 0, ctx->stream, d_sum, d_tot, d_wins,
                               m->compact ? m->d_onesmap : nullptr, N, min_run, d_rec, d_ind, ctx->d_err);
        }))) return rc;
        ++launches;
        if (ind_out)
            HIP_TRY(hipMemcpyAsync(ind_out + c.w_begin * N, d_ind, cnt * N * sizeof(impop_diploid_ind), hipMemcpyDeviceToHost, ctx->stream));
        if ((rc = run.finish(o_rec, o_rec + cnt * sizeof(impop_diploid_stats)))) return rc;
        const impop_diploid_stats *rv = (const impop_diploid_stats *)(hc + o_rec);
        const double nan = __builtin_nan("");
        for (size_t k = 0; k < cnt; ++k) {
            impop_diploid_stats o = rv[k];
            const uint64_t seq_len = windows[c.w_begin + k].seq_len, W = o.n_sites, nn = 2ull * N;
            const double Ld = (double)(seq_len > 0 ? seq_len : W);
            o.ho = (double)o.het_total / ((double)N * Ld);
            o.he = 2.0 * (double)o.sum_p / ((double)nn * (double)(nn - 1) * Ld);
            o.f_is = o.sum_p == 0 ? nan : 1.0 - (double)(o.het_total * (nn - 1)) / (double)o.sum_p;
            o.f_roh = W == 0 ? nan : (double)o.roh_sites_total / ((double)N * (double)W);
            out_host[c.w_begin + k] = o;
        }
        tiles_run += nt;
    }
    if (trace_on()) {
        fprintf(stderr, "[impop_diploid_scan] route=%s windows=%llu tiles=%llu chunks=%llu launches=%llu individuals=%u bytes_streamed=%llu\n",
                m->compact ? "compact" : "dense", (unsigned long long)n_windows, (unsigned long long)tiles_run,
                (unsigned long long)chunks.size(), (unsigned long long)launches, N, (unsigned long long)bytes_streamed);
        fflush(stderr);
    }
    return IMPOP_OK;
}

IMPOP_API int impop_ctx_diploid_elapsed(impop_ctx *ctx, double kernel_ms[2], uint64_t *chunks) {
    REQUIRE(ctx && kernel_ms, "impop_ctx_diploid_elapsed: NULL argument");
    return ctx_timers_elapsed(ctx, impop_ctx::T_DIP, 2, 1, kernel_ms, chunks);
}
