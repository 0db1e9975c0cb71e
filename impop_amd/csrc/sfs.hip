// sfs.hip — impop_sfs_scan: what is read from the site-frequency spectrum, per window (include/impop_hip.h): every population's
// spectrum summaries and neutrality statistics, every requested pair's Wakeley-Hey site classes, and optionally the 1-D and the
// joint spectra as tables.  Both passes stream what scan_route picks through pop_stream.h, like dstat.hip: masks in LDS, a lane
// per site, the rare entries of a split index.  Every term is zero where the site is monomorphic among all haplotypes (no
// population segregates there, and an outgroup count of 0 or nO is never a tie), so the sites the index and a compaction drop add
// nothing, with or without polarisation.
//
// Summary pass: per population two 64-bit sums (sum c, sum c^2 over its segregating sites; sum c (n - c) = n sum c - sum c^2 is
// formed from the two window totals, exactly, so it costs no registers) and three counters, per pair five counters, one tie
// counter; per-tile integer partials, a finalize kernel adds each window's tile range.  The pair list is handled
// IMPOP_SFS_PAIR_GROUP at a time, all populations in the first launch (DESIGN.md has the register report).  The doubles of a
// record are computed on the host from its integers, in one place (sfs_math.h).
//
// Table pass: one job per requested table, streaming the job's own 1..3 populations (the population or the pair, plus the
// outgroup).  A workgroup owns a (window, part) item, walks the part's tiles and tallies into a histogram in LDS, then adds its
// non-zero bins to the window's zero-initialised table with integer atomicAdd (the order of integer adds cannot change a table);
// a job whose bins do not fit the LDS tallies straight into the table.  Tables come down per chunk of windows.
#include <string.h>

#include <algorithm>
#include <vector>

#include "device_utils.h"
#include "internal.h"
#include "pop_stream.h"
#include "scan_route.h"
#include "sfs_math.h"
#include "win_chunks.h"

namespace impop {

constexpr int SFS_PG = (int)IMPOP_SFS_PAIR_GROUP;  // pairs per launch
constexpr int SFS_POP_NV = 5;                      // per population and tile: sum_c, sum_c2, seg, eta1, eta_n1
constexpr int SFS_PAIR_NV = 5;                     // per pair and tile: private_a, private_b, shared, fixed_a, fixed_b
constexpr uint32_t SFS_PART_TILES = 4;             // tiles of a (window, part) item of the table pass
constexpr uint32_t SFS_LDS_BYTES = 160u * 1024u;   // a workgroup's LDS
constexpr uint32_t SFS_NONE = 0xFFFFFFFFu;

struct SfsPanel {  // a kernel argument: wave-uniform (SGPR) state
    uint32_t n[8];           // population sizes
    uint32_t outgroup;       // SFS_NONE: none
    uint32_t pa[SFS_PG], pb[SFS_PG];  // the group's pairs, indices into the K populations
};

struct SfsPopAcc {
    uint64_t c = 0, c2 = 0;
    uint32_t seg = 0, eta1 = 0, eta_n1 = 0;
};
struct SfsPairAcc {
    uint32_t v[SFS_PAIR_NV] = {0, 0, 0, 0, 0};
};

// The counts of a site as the outgroup polarises them.  Returns false for a tie.
template <int K>
__device__ __forceinline__ bool sfs_polarize(const uint32_t (&c)[K], const uint32_t (&n)[K], uint32_t outgroup,
                                             uint32_t (&cc)[K]) {
    bool flip = false, tie = false;
    if (outgroup != SFS_NONE) {  // wave-uniform
        const uint32_t cO = dstat_pick(c, outgroup), nO = dstat_pick(n, outgroup);
        flip = 2u * cO > nO;
        tie = 2u * cO == nO;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) cc[k] = flip ? n[k] - c[k] : c[k];
    return !tie;
}

// grid = tiles, block = 256.  Dynamic LDS: the K masks, wps4 dwords each.  with_pops: the launch carries the populations'
// accumulators (the first pair group's does); nq <= SFS_PG pairs of pn are meaningful.
// out: tile-major, 1 + K x SFS_POP_NV + SFS_PG x SFS_PAIR_NV uint64 per tile, the tie counter first.
template <int K, bool WEIGHTED>
__global__ __launch_bounds__(256, 2) void sfs_tiles_kernel(const uint32_t *__restrict__ sb, const uint64_t *__restrict__ rare,
                                                           const ScanTile *__restrict__ tiles,
                                                           const uint32_t *__restrict__ masks /* K x wps */,
                                                           const uint32_t *__restrict__ pop_n /* K */, uint32_t wps, uint32_t G,
                                                           uint32_t r, const uint32_t *__restrict__ weights /* WEIGHTED */,
                                                           SfsPanel pn, uint32_t nq, int with_pops, uint64_t *__restrict__ out) {
    constexpr int NV = 1 + K * SFS_POP_NV + SFS_PG * SFS_PAIR_NV;
    extern __shared__ __attribute__((aligned(16))) uint32_t mk_lds[];  // K x wps4
    pop_masks_to_lds<K>(mk_lds, masks, wps);
    __syncthreads();
    const ScanTile t = tiles[blockIdx.x];
    const TileBlocks tb = tile_blocks_of(t);
    uint32_t n[K];
#pragma unroll
    for (int k = 0; k < K; ++k) n[k] = pn.n[k];
    SfsPopAcc pop[K];
    SfsPairAcc pair[SFS_PG];
    uint32_t skipped = 0;
    auto tally_counts = [&](const uint32_t (&c)[K], uint32_t wt) {
        uint32_t cc[K];
        const bool use = sfs_polarize(c, n, pn.outgroup, cc);
        skipped += !use;
        if (with_pops) {  // wave-uniform
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const uint32_t ck = cc[k];
                const bool seg = use && ck != 0u && ck != n[k];
                const uint32_t cs = seg ? ck : 0u;  // c <= 65535: c^2 fits 32 bits
                pop[k].seg += seg;
                pop[k].eta1 += seg && ck == 1u;
                pop[k].eta_n1 += seg && ck + 1u == n[k];
                if (WEIGHTED) {
                    pop[k].c += (uint64_t)wt * cs;
                    pop[k].c2 += (uint64_t)wt * (cs * cs);
                } else {
                    pop[k].c += cs;
                    pop[k].c2 += cs * cs;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < SFS_PG; ++j) {
            if ((uint32_t)j >= nq) continue;  // wave-uniform: a short group
            const uint32_t ca = dstat_pick(cc, pn.pa[j]), cb = dstat_pick(cc, pn.pb[j]);
            const uint32_t na = dstat_pick(n, pn.pa[j]), nb = dstat_pick(n, pn.pb[j]);
            const bool sa = ca != 0u && ca != na, sb_ = cb != 0u && cb != nb;
            pair[j].v[0] += use && sa && !sb_;
            pair[j].v[1] += use && !sa && sb_;
            pair[j].v[2] += use && sa && sb_;
            pair[j].v[3] += use && ca == na && cb == 0u;
            pair[j].v[4] += use && ca == 0u && cb == nb;
        }
    };
    // the rare entries of the split index belong to unweighted matrices only: compiled out under WEIGHTED
    pop_stream_tile<K, !WEIGHTED>(
        sb, rare, t, tb, mk_lds, pop_n, wps, G, r, [&](const uint32_t (&c)[K], uint64_t s) { tally_counts(c, WEIGHTED ? weights[s] : 1u); },
        [&](const uint32_t (&c)[K]) { tally_counts(c, 1u); });
    tile_partials_store<NV>(tb, out, [&](int i) -> uint64_t {
        if (i == 0) return wave_sum_u32(skipped);
        if (i < 1 + K * SFS_POP_NV) {  // i is a constant once the caller's loop is unrolled
            const SfsPopAcc &a = pop[(i - 1) / SFS_POP_NV];
            switch ((i - 1) % SFS_POP_NV) {
                case 0: return wave_sum_u64(a.c);
                case 1: return wave_sum_u64(a.c2);
                case 2: return wave_sum_u32(a.seg);
                case 3: return wave_sum_u32(a.eta1);
                default: return wave_sum_u32(a.eta_n1);
            }
        }
        const int j = i - 1 - K * SFS_POP_NV;
        return wave_sum_u32(pair[j / SFS_PAIR_NV].v[j % SFS_PAIR_NV]);
    });
}

// one thread per (window, slot): slot < n_rec_pops is a population (K in the first launch, else 0), the others the group's pairs.
// The window's tile range added up, the record's integers written.
__global__ __launch_bounds__(128) void sfs_finalize_kernel(const uint64_t *__restrict__ parts, const WinDesc *__restrict__ wins,
                                                           uint64_t n_windows, uint32_t K, uint32_t n_rec_pops, uint32_t nq,
                                                           uint32_t q0, uint32_t n_pairs, SfsPanel pn,
                                                           impop_sfs_stats *__restrict__ stats_out,
                                                           impop_sfs_pair *__restrict__ pairs_out) {
    const uint32_t slots = n_rec_pops + nq;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_windows * slots) return;
    const uint64_t win = i / slots;
    const uint32_t slot = (uint32_t)(i % slots);
    const WinDesc w = wins[win];
    const uint32_t NV = 1 + K * SFS_POP_NV + SFS_PG * SFS_PAIR_NV;
    const bool is_pop = slot < n_rec_pops;
    const uint32_t first = is_pop ? 1 + slot * SFS_POP_NV : 1 + K * SFS_POP_NV + (slot - n_rec_pops) * SFS_PAIR_NV;
    uint64_t s[5] = {0, 0, 0, 0, 0}, skipped = 0;
    for (uint64_t t = w.t0; t < w.t1; ++t) {
        const uint64_t *p = parts + t * NV;
        skipped += p[0];
#pragma unroll
        for (int f = 0; f < 5; ++f) s[f] += p[first + f];
    }
    if (is_pop) {
        impop_sfs_stats o;
        o.n_sites = (uint32_t)w.n_sites;
        o.seg = (uint32_t)s[2];
        o.eta1 = (uint32_t)s[3];
        o.eta_n1 = (uint32_t)s[4];
        o.n_skipped = (uint32_t)skipped;
        o.flags = 0;
        o.sum_c = s[0];
        o.sum_c2 = s[1];
        o.sum_het = (uint64_t)pn.n[slot] * s[0] - s[1];  // sum c (n - c), exact: n sum_c < 2^62 by the call's overflow check
        o.theta_w = o.theta_pi = o.theta_h = o.theta_l = o.tajima_d = o.faywu_h = o.faywu_h_norm = o.zeng_e = 0.0;  // the host's
        stats_out[win * K + slot] = o;
    } else {
        impop_sfs_pair o;
        o.private_a = (uint32_t)s[0];
        o.private_b = (uint32_t)s[1];
        o.shared = (uint32_t)s[2];
        o.fixed_a = (uint32_t)s[3];
        o.fixed_b = (uint32_t)s[4];
        o.n_union = (uint32_t)(s[0] + s[1] + s[2] + s[3] + s[4]);
        o.n_skipped = (uint32_t)skipped;
        o.flags = 0;
        pairs_out[win * n_pairs + q0 + (slot - n_rec_pops)] = o;
    }
}

// ---- the table pass
struct SfsJob {  // a kernel argument
    uint32_t pop[3];   // the populations streamed: the table's one or two, then the outgroup (if any)
    uint32_t n[3];     // their sizes
    uint32_t bins;     // n0 + 1, or (n0 + 1) (n1 + 1)
    uint32_t hot[2];   // the bins singletons land in: counted per wave
    uint64_t row_off;  // the table's place in a window's row
    uint64_t row_len;  // the row's length
};

// grid = the chunk's items, block = 256.  KJ populations streamed; JOINT: a pair's joint table, else a population's spectrum; the
// outgroup is the last of the KJ when KJ - JOINT == 2.  Dynamic LDS: the KJ masks, then (LDS_FORM) the job's bins.
// table: the chunk's rows of tables, zero before the first job.
template <int KJ, bool JOINT, bool LDS_FORM>
__global__ __launch_bounds__(256) void sfs_table_kernel(const uint32_t *__restrict__ sb, const uint64_t *__restrict__ rare,
                                                        const ScanTile *__restrict__ tiles, const uint32_t *__restrict__ masks,
                                                        const uint32_t *__restrict__ job_n /* KJ */, uint32_t wps, uint32_t G, uint32_t r,
                                                        SfsJob job, const SfsItem *__restrict__ items, uint32_t *__restrict__ table) {
    constexpr bool POLARIZED = KJ - (JOINT ? 1 : 0) == 2;
    extern __shared__ __attribute__((aligned(16))) uint32_t mk_lds[];  // KJ x wps4, then the histogram
    const uint32_t wps4 = (wps + 3) & ~3u;
    for (uint32_t i = threadIdx.x; i < KJ * wps4; i += 256) {
        const uint32_t k = i / wps4, j = i % wps4;
        mk_lds[i] = j < wps ? masks[(uint64_t)job.pop[k] * wps + j] : 0u;
    }
    const SfsItem it = items[blockIdx.x];
    uint32_t *const row = table + (uint64_t)it.win * job.row_len + job.row_off;
    uint32_t *const hist_lds = mk_lds + KJ * wps4;
    if (LDS_FORM)
        for (uint32_t i = threadIdx.x; i < job.bins; i += 256) hist_lds[i] = 0u;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t n0 = job.n[0], n1 = job.n[1], nO = job.n[KJ - 1];
    auto add = [&](uint32_t bin, uint32_t v) {
        if (LDS_FORM) atomicAdd(hist_lds + bin, v);
        else atomicAdd(row + bin, v);
    };
    // the lanes of a wave that run this together and hold a hot bin add it once (64 lanes adding to one word serialise, and on
    // the index routes most sites are singletons); every other bin by its own lane
    auto tally = [&](const uint32_t (&c)[KJ]) {
        uint32_t c0 = c[0], c1 = JOINT ? c[1] : 0u;
        bool use = true;
        if (POLARIZED) {
            const uint32_t cO = c[KJ - 1];
            use = 2u * cO != nO;
            if (2u * cO > nO) {
                c0 = n0 - c0;
                if (JOINT) c1 = n1 - c1;
            }
        }
        uint32_t bin;
        if (JOINT) {
            use = use && (c0 | c1) != 0u && !(c0 == n0 && c1 == n1);
            bin = c0 * (n1 + 1u) + c1;
        } else {
            use = use && c0 != 0u && c0 != n0;
            bin = c0;
        }
        const uint64_t h0 = __ballot(use && bin == job.hot[0]), h1 = __ballot(use && bin == job.hot[1] && bin != job.hot[0]);
        if (h0 && lane == (uint32_t)__ffsll((unsigned long long)h0) - 1u) add(job.hot[0], (uint32_t)__popcll(h0));
        if (h1 && lane == (uint32_t)__ffsll((unsigned long long)h1) - 1u) add(job.hot[1], (uint32_t)__popcll(h1));
        if (use && bin != job.hot[0] && bin != job.hot[1]) add(bin, 1u);
    };
    for (uint32_t ti = it.t0; ti < it.t1; ++ti) {
        const ScanTile t = tiles[ti];
        const TileBlocks tb = tile_blocks_of(t);
        pop_stream_tile<KJ, true>(
            sb, rare, t, tb, mk_lds, job_n, wps, G, r, [&](const uint32_t (&c)[KJ], uint64_t) { tally(c); },
            [&](const uint32_t (&c)[KJ]) { tally(c); });
    }
    if (LDS_FORM) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < job.bins; i += 256) {
            const uint32_t v = hist_lds[i];
            if (v) atomicAdd(row + i, v);
        }
    }
}

// IMPOP_SFS_TILE_BLOCKS=n (1..4096) overrides the tile size, so that tests reach many-tile windows on small matrices; it beats
// params->tile_blocks (0: the default)
static uint32_t sfs_tile_blocks(const impop_sfs_params *params) {
    const uint32_t e = env_tile_blocks("IMPOP_SFS_TILE_BLOCKS");
    return e ? e : std::min<uint32_t>(params->tile_blocks, 4096u);
}
// the bins a job's histogram may have to take the LDS form: what the LDS holds next to the job's masks, or IMPOP_SFS_LDS_BINS=n
// (0..40960) where that is less, so that tests reach the global form at small sizes
static uint32_t sfs_lds_bins(uint32_t kj, uint32_t wps) {
    const uint32_t mask_bytes = kj * ((wps + 3) & ~3u) * 4u;
    uint32_t cap = mask_bytes < SFS_LDS_BYTES ? (SFS_LDS_BYTES - mask_bytes) / 4u : 0u;
    const char *e = getenv("IMPOP_SFS_LDS_BINS");
    if (e && *e) {
        const long v = strtol(e, nullptr, 10);
        cap = std::min<uint32_t>(cap, v < 0 ? 0u : v > 40960 ? 40960u : (uint32_t)v);
    }
    return cap;
}

struct SfsTableJob {
    SfsJob job;
    uint32_t kj;
    bool joint, lds;  // lds: the job's bins fit the LDS next to its masks
    int region;  // 0: the 1-D rows, 1: the joint rows
};

template <int KJ, bool JOINT>
static int sfs_launch_table(bool lds_form, hipStream_t st, const impop_matrix *m, const ScanRoute &rt, const PopPanelDev &dev,
                            const uint32_t *job_n, const SfsJob &job, const SfsItem *items, uint32_t n_items, uint32_t *table) {
    const size_t lds = (size_t)KJ * ((m->g.wps + 3) & ~3u) * 4 + (lds_form ? (size_t)job.bins * 4 : 0);
    if (lds_form) {
        const int rc = lds_opt_in(sfs_table_kernel<KJ, JOINT, true>, lds);
        if (rc) return rc;
        hipLaunchKernelGGL((sfs_table_kernel<KJ, JOINT, true>), dim3(n_items), dim3(256), lds, st, rt.sb, rt.rare,
                           (const ScanTile *)dev.tiles, (const uint32_t *)dev.masks, job_n, m->g.wps, m->g.G, m->g.r, job, items, table);
    } else {
        const int rc = lds_opt_in(sfs_table_kernel<KJ, JOINT, false>, lds);
        if (rc) return rc;
        hipLaunchKernelGGL((sfs_table_kernel<KJ, JOINT, false>), dim3(n_items), dim3(256), lds, st, rt.sb, rt.rare,
                           (const ScanTile *)dev.tiles, (const uint32_t *)dev.masks, job_n, m->g.wps, m->g.G, m->g.r, job, items, table);
    }
    HIP_TRY(hipGetLastError());
    return IMPOP_OK;
}

}  // namespace impop

using namespace impop;

IMPOP_API int impop_sfs_neutrality(uint32_t n, uint64_t seg, uint64_t sum_het, uint64_t sum_c, uint64_t sum_c2, double out[8]) {
    REQUIRE(out, "impop_sfs_neutrality: out is NULL");
    const TajConsts c = tajima_consts(n >= 2 ? (int64_t)n : 2);
    sfs_neutrality(sfs_consts(n, c.a1, c.a2, c.e1, c.e2), seg, sum_het, sum_c, sum_c2, out);
    return IMPOP_OK;
}

IMPOP_API int impop_sfs_scan(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows,
                             const uint64_t *masks, uint32_t n_pop, const uint32_t *pairs, uint32_t n_pairs,
                             const impop_sfs_params *params, impop_sfs_stats *stats_out, impop_sfs_pair *pairs_out, uint32_t *sfs_out,
                             uint32_t *jsfs_out) {
    static_assert(sizeof(impop_sfs_stats) == 112 && sizeof(impop_sfs_pair) == 32 && sizeof(impop_sfs_params) == 24, "ABI layout");
    const char *fn = "impop_sfs_scan";
    REQUIRE(ctx && m && params, "%s: NULL argument", fn);
    REQUIRE(params->struct_size == sizeof(impop_sfs_params), "impop_sfs_params.struct_size mismatch");
    REQUIRE(m->device == ctx->device, "%s: matrix lives on device %d, context on %d", fn, m->device, ctx->device);
    REQUIRE(n_pop >= 1 && n_pop <= 8, "%s: n_pop must be 1..8 (got %u)", fn, n_pop);
    REQUIRE(masks, "%s: masks is NULL", fn);
    REQUIRE(n_pairs <= IMPOP_SFS_MAX_PAIRS, "%s: n_pairs must be 0..%u (got %u)", fn, IMPOP_SFS_MAX_PAIRS, n_pairs);
    REQUIRE(!n_pairs || pairs, "%s: pairs is NULL", fn);
    REQUIRE(m->g.n_hap <= 65535, "%s: n_hap > 65535 not supported", fn);
    const uint32_t wps = m->g.wps, K = n_pop, Q = n_pairs;
    REQUIRE(params->outgroup >= -1 && params->outgroup < (int32_t)K, "%s: outgroup %d outside the %u populations (-1: none)", fn,
            params->outgroup, K);
    const uint32_t outgroup = params->outgroup < 0 ? SFS_NONE : (uint32_t)params->outgroup;
    const bool want_sfs = (params->tables & IMPOP_SFS_TABLE_1D) != 0, want_jsfs = (params->tables & IMPOP_SFS_TABLE_JOINT) != 0;
    REQUIRE((params->tables & ~(IMPOP_SFS_TABLE_1D | IMPOP_SFS_TABLE_JOINT)) == 0, "%s: unknown tables bits 0x%x", fn, params->tables);
    REQUIRE(!want_jsfs || Q, "%s: the joint spectra (tables bit 1) need at least one pair", fn);
    REQUIRE(!want_sfs || sfs_out, "%s: tables bit 0 is set and sfs_out is NULL", fn);
    REQUIRE(!want_jsfs || jsfs_out, "%s: tables bit 1 is set and jsfs_out is NULL", fn);
    PopPanel panel;
    pop_panel_pack(m, masks, K, panel);
    const std::vector<uint32_t> &mk = panel.mk, &nk = panel.nk;
    for (uint32_t k = 0; k < K; ++k) REQUIRE(nk[k] > 0, "%s: population %u is empty", fn, k);
    for (uint32_t q = 0; q < Q; ++q) {
        const uint32_t a = pairs[2 * q], b = pairs[2 * q + 1];
        REQUIRE(a < K && b < K, "%s: pair %u: population index %u outside the %u populations", fn, q, a < K ? b : a, K);
        REQUIRE(a != b, "%s: pair %u: both populations are %u", fn, q, a);
        for (uint32_t j = 0; j < wps; ++j)
            REQUIRE((mk[(size_t)a * wps + j] & mk[(size_t)b * wps + j]) == 0u,
                    "%s: pair %u: populations %u and %u share a haplotype (the two populations of a pair must be disjoint)", fn, q, a, b);
    }
    int rc = check_windows(fn, m, windows, windows ? n_windows : 0);
    if (rc) return rc;
    if (!n_windows) return IMPOP_OK;
    REQUIRE(windows && stats_out, "%s: NULL windows/stats_out", fn);
    REQUIRE(!Q || pairs_out, "%s: pairs_out is NULL", fn);
    // no sum can wrap: a term is at most n^2 / 4 < n^2 (sum_c2: n^2), a window adds at most its weight sum of them
    uint64_t w_max = 0, w_arg = 0;
    for (uint64_t i = 0; i < n_windows; ++i) {
        const uint64_t W = window_W(m, windows[i].site_begin, windows[i].site_end);
        if (W > w_max) { w_max = W; w_arg = i; }
    }
    for (uint32_t k = 0; k < K; ++k)
        if ((unsigned __int128)((uint64_t)nk[k] * nk[k]) * w_max >= ((unsigned __int128)1 << 62)) {
            set_error("%s: population %u (size %u) over window %llu (weight sum %llu): n^2 W is not below 2^62, the sums could wrap; "
                      "split the window",
                      fn, k, nk[k], (unsigned long long)w_arg, (unsigned long long)w_max);
            return IMPOP_E_UNSUPPORTED;
        }
    const SfsTableRows rows = sfs_table_rows(nk.data(), K, pairs, Q);
    const uint64_t sfs_len = want_sfs ? rows.sfs_off[K] : 0, jsfs_len = want_jsfs ? rows.jsfs_off[Q] : 0;

    HIP_TRY(hipSetDevice(ctx->device));
    ScanRoute rt;
    rc = scan_route(fn, ctx, m, windows, n_windows, sfs_tile_blocks(params), rt);
    if (rc) return rc;
    const size_t nt = rt.tiles.size();

    // the table pass's jobs, and its chunks of windows: a chunk holds its windows' rows of tables and its items
    std::vector<SfsTableJob> jobs;
    auto add_job = [&](uint32_t a, uint32_t b /* SFS_NONE: a 1-D spectrum */, uint64_t off, uint64_t len, int region) {
        SfsTableJob j;
        memset(&j.job, 0, sizeof(j.job));
        j.joint = b != SFS_NONE;
        uint32_t kj = 0;
        j.job.pop[kj++] = a;
        if (j.joint) j.job.pop[kj++] = b;
        if (outgroup != SFS_NONE) j.job.pop[kj++] = outgroup;
        for (uint32_t i = 0; i < 3; ++i) j.job.n[i] = i < kj ? nk[j.job.pop[i]] : 0u;
        j.kj = kj;
        if (j.joint) {
            j.job.bins = (nk[a] + 1) * (nk[b] + 1);
            j.job.hot[0] = (uint32_t)sfs_joint_bin(1, 0, nk[b]);
            j.job.hot[1] = (uint32_t)sfs_joint_bin(0, 1, nk[b]);
        } else {
            j.job.bins = nk[a] + 1;
            j.job.hot[0] = 1;
            j.job.hot[1] = nk[a] - 1;
        }
        j.job.row_off = off;
        j.job.row_len = len;
        j.lds = j.job.bins <= sfs_lds_bins(kj, wps);
        j.region = region;
        jobs.push_back(j);
    };
    if (want_sfs)
        for (uint32_t k = 0; k < K; ++k) add_job(k, SFS_NONE, rows.sfs_off[k], sfs_len, 0);
    if (want_jsfs)
        for (uint32_t q = 0; q < Q; ++q) add_job(pairs[2 * q], pairs[2 * q + 1], rows.jsfs_off[q], jsfs_len, 1);
    std::vector<WinChunk> chunks;
    size_t max_items = 0, max_wins = 0;
    if (!jobs.empty()) {
        const uint64_t row_bytes = (sfs_len + jsfs_len) * 4;
        chunks = cut_windows(n_windows, chunk_budget(params->max_chunk_bytes), 0xFFFFFFFFull, [&](size_t, uint64_t i) {
            return row_bytes + sfs_part_count(rt.wins[i].t1 - rt.wins[i].t0, SFS_PART_TILES) * sizeof(SfsItem);
        });
        for (const WinChunk &c : chunks) {
            size_t items = 0;
            for (uint64_t i = c.w_begin; i < c.w_end; ++i) items += sfs_part_count(rt.wins[i].t1 - rt.wins[i].t0, SFS_PART_TILES);
            max_items = std::max(max_items, items);
            max_wins = std::max<size_t>(max_wins, c.w_end - c.w_begin);
        }
        REQUIRE(max_items < 0x7FFFFFFFull, "%s: %llu table items exceed one launch; lower max_chunk_bytes", fn, (unsigned long long)max_items);
    }

    constexpr size_t NV_MAX = 1 + 8 * SFS_POP_NV + SFS_PG * SFS_PAIR_NV;
    const size_t NV = 1 + (size_t)K * SFS_POP_NV + SFS_PG * SFS_PAIR_NV;
    static_assert(NV_MAX <= 256, "tile_partials_store writes a tile's row with one thread per value");
    PopPanelDev dev;
    uint64_t *dp = nullptr;
    impop_sfs_stats *d_stats = nullptr;
    impop_sfs_pair *d_pairs = nullptr;
    uint32_t *d_job_n = nullptr, *d_sfs = nullptr, *d_jsfs = nullptr;
    SfsItem *d_items = nullptr;
    rc = pop_panel_upload(ctx, rt, panel, dev, [&](Layout &L) {
        L.sub(dp, std::max<size_t>(nt, 1) * NV);
        L.sub(d_stats, n_windows * K);
        L.sub(d_pairs, n_windows * Q);
        L.sub(d_job_n, std::max<size_t>(jobs.size(), 1) * 4);
        L.sub(d_items, std::max<size_t>(max_items, 1));
        L.sub(d_sfs, max_wins * sfs_len);
        L.sub(d_jsfs, max_wins * jsfs_len);
    });
    if (rc) return rc;
    const uint32_t *weights = m->d_wt && !rt.indexed ? m->d_wt : nullptr;  // weighted matrices stream their rows
    EventPairs *timer = &ctx->timers[impop_ctx::T_SFS];
    SfsPanel pn;
    memset(&pn, 0, sizeof(pn));
    for (uint32_t k = 0; k < K; ++k) pn.n[k] = nk[k];
    pn.outgroup = outgroup;
    uint64_t launches = 0;
    // the pair list in groups of SFS_PG: the same tiles, the partials reused (the launches of a stream run in order); the
    // populations ride with the first group, which runs even without pairs
    for (uint32_t q0 = 0; q0 == 0 || q0 < Q; q0 += SFS_PG) {
        const uint32_t nq = Q > q0 ? std::min<uint32_t>(SFS_PG, Q - q0) : 0u;
        const int with_pops = q0 == 0;
        for (uint32_t j = 0; j < (uint32_t)SFS_PG; ++j) {  // a short group repeats its first pair (or population 0)
            const uint32_t q = nq ? q0 + (j < nq ? j : 0) : 0;
            pn.pa[j] = nq ? pairs[2 * q] : 0u;
            pn.pb[j] = nq ? pairs[2 * q + 1] : 0u;
        }
        if (nt) {
            rc = timed(ctx, timer[0], [&] {
                return pop_dispatch_k<1>(K, [&](auto k) {
                    return weights ? pop_launch(sfs_tiles_kernel<k.value, true>, K, ctx->stream, m, rt, dev, weights, pn, nq, with_pops, dp)
                                   : pop_launch(sfs_tiles_kernel<k.value, false>, K, ctx->stream, m, rt, dev, weights, pn, nq, with_pops, dp);
                });
            });
            if (rc) return rc;
            ++launches;
        }
        const uint32_t n_rec_pops = with_pops ? K : 0u;
        const uint64_t slots = n_windows * (n_rec_pops + nq);
        if (slots) {
            hipLaunchKernelGGL(sfs_finalize_kernel, dim3((uint32_t)((slots + 127) / 128)), dim3(128), 0, ctx->stream, (const uint64_t *)dp,
                               (const WinDesc *)dev.wins, n_windows, K, n_rec_pops, nq, q0, Q, pn, d_stats, d_pairs);
            HIP_TRY(hipGetLastError());
            ++launches;
        }
    }
    HIP_TRY(hipMemcpyAsync(stats_out, d_stats, n_windows * K * sizeof(impop_sfs_stats), hipMemcpyDeviceToHost, ctx->stream));
    if (Q) HIP_TRY(hipMemcpyAsync(pairs_out, d_pairs, n_windows * Q * sizeof(impop_sfs_pair), hipMemcpyDeviceToHost, ctx->stream));

    // the table pass, a chunk of windows at a time: items up through the page-locked staging, the rows zeroed, one launch per
    // job, the rows down into the caller's tables
    uint64_t table_items = 0, table_bytes = 0, lds_jobs = 0;
    for (const SfsTableJob &j : jobs) lds_jobs += j.lds;
    if (!jobs.empty()) {
        std::vector<uint32_t> job_n(jobs.size() * 4, 0u);
        for (size_t j = 0; j < jobs.size(); ++j)
            for (uint32_t i = 0; i < 3; ++i) job_n[4 * j + i] = jobs[j].job.n[i];
        HIP_TRY(hipMemcpyAsync(d_job_n, job_n.data(), job_n.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));  // job_n is pageable and leaves scope
        void *pin = nullptr;
        rc = ctx_pinned(ctx, std::max<size_t>(max_items, 1) * sizeof(SfsItem), &pin);
        if (rc) return rc;
        const ChunkRun run{ctx, fn, (char *)d_items, (char *)pin};
        std::vector<SfsItem> items;
        for (const WinChunk &c : chunks) {
            const size_t cnt = c.w_end - c.w_begin;
            items.clear();
            sfs_cut_parts(rt.wins.data(), c.w_begin, c.w_end, SFS_PART_TILES, items);
            if (sfs_len) HIP_TRY(hipMemsetAsync(d_sfs, 0, cnt * sfs_len * 4, ctx->stream));
            if (jsfs_len) HIP_TRY(hipMemsetAsync(d_jsfs, 0, cnt * jsfs_len * 4, ctx->stream));
            if (!items.empty()) {
                memcpy(pin, items.data(), items.size() * sizeof(SfsItem));
                if ((rc = run.up(0, items.size() * sizeof(SfsItem)))) return rc;
                uint64_t item_bytes = 0;
                for (const SfsItem &it : items)
                    for (uint32_t t = it.t0; t < it.t1; ++t) item_bytes += tile_bytes_streamed(rt.tiles[t], wps);
                for (size_t j = 0; j < jobs.size(); ++j) {
                    const SfsTableJob &tj = jobs[j];
                    uint32_t *table = tj.region ? d_jsfs : d_sfs;
                    const uint32_t *jn = d_job_n + 4 * j;
                    const uint32_t ni = (uint32_t)items.size();
                    rc = run.timed(timer[1], [&] {
                        if (tj.joint)
                            return tj.kj == 3 ? sfs_launch_table<3, true>(tj.lds, ctx->stream, m, rt, dev, jn, tj.job, d_items, ni, table)
                                              : sfs_launch_table<2, true>(tj.lds, ctx->stream, m, rt, dev, jn, tj.job, d_items, ni, table);
                        return tj.kj == 2 ? sfs_launch_table<2, false>(tj.lds, ctx->stream, m, rt, dev, jn, tj.job, d_items, ni, table)
                                          : sfs_launch_table<1, false>(tj.lds, ctx->stream, m, rt, dev, jn, tj.job, d_items, ni, table);
                    });
                    if (rc) return rc;
                    ++launches;
                    table_bytes += item_bytes;
                }
                table_items += items.size();
            }
            if (sfs_len) HIP_TRY(hipMemcpyAsync(sfs_out + c.w_begin * sfs_len, d_sfs, cnt * sfs_len * 4, hipMemcpyDeviceToHost, ctx->stream));
            if (jsfs_len)
                HIP_TRY(hipMemcpyAsync(jsfs_out + c.w_begin * jsfs_len, d_jsfs, cnt * jsfs_len * 4, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));  // the next chunk reuses the staging and the rows
        }
    }
    rc = ctx_err_fetch(ctx);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    rc = ctx_err_result(ctx, fn);
    if (rc) return rc;
    std::vector<SfsConsts> consts(K);  // what the doubles need of a population's size, once
    for (uint32_t k = 0; k < K; ++k) {
        const TajConsts t = tajima_consts(nk[k] >= 2 ? (int64_t)nk[k] : 2);
        consts[k] = sfs_consts(nk[k], t.a1, t.a2, t.e1, t.e2);
    }
    for (uint64_t i = 0; i < n_windows; ++i)
        for (uint32_t k = 0; k < K; ++k) {
            impop_sfs_stats &o = stats_out[i * K + k];
            sfs_neutrality(consts[k], o.seg, o.sum_het, o.sum_c, o.sum_c2, &o.theta_w);
        }
    if (trace_on()) {
        fprintf(stderr,
                "[impop_sfs_scan] route=%s windows=%llu tiles=%llu pops=%u pairs=%u launches=%llu table_jobs=%llu lds_jobs=%llu "
                "table_items=%llu chunks=%llu bytes_streamed=%llu table_bytes_streamed=%llu\n",
                rt.split ? "indexed+rare" : rt.indexed ? "indexed" : m->compact ? "compact" : "dense", (unsigned long long)n_windows,
                (unsigned long long)nt, K, Q, (unsigned long long)launches, (unsigned long long)jobs.size(), (unsigned long long)lds_jobs,
                (unsigned long long)table_items, (unsigned long long)chunks.size(), (unsigned long long)rt.bytes_streamed,
                (unsigned long long)table_bytes);
        fflush(stderr);
    }
    return IMPOP_OK;
}

IMPOP_API int impop_ctx_sfs_elapsed(impop_ctx *ctx, double kernel_ms[2], uint64_t *launches) {
    REQUIRE(ctx, "impop_ctx_sfs_elapsed: ctx is NULL");
    return ctx_timers_elapsed(ctx, impop_ctx::T_SFS, 2, 0, kernel_ms, launches);
}
