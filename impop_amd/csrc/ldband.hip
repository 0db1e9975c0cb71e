// ldband.hip — impop_ldband_scan: r2 between every qualifying site of a window and its next band_sites qualifying neighbours, no
// thinning, and from that one banded pass the LD decay curve, per-site LD scores and a greedy LD pruning.  r2 leaves the pair
// arithmetic as a fixed-point integer (ldband_math.h), so every device output is an integer and any order of the atomics gives
// the same bytes (contract: include/impop_hip.h, impop_ldband_scan).
//
// Site selection is impop_ld_scan's (ld_select.h, ld_select_kernel).  q is not known before it has run, and the call must refuse a
// window that cannot fit before it writes anything, so the call has two phases:
//   count   per chunk of windows cut by their mask bytes: ld_select_kernel, ldband_rank_kernel, one copy of the q's to the host.
//   work    chunks cut from the real q: a window's slots in the chunk's scratch number q and start at the prefix of the q's before
//           it, so that a dense chromosome costs what qualifies, not its length.  Per chunk, six launches:
//   1. ld_select_kernel      the qualifying mask of every 64-site block                                       (streams the rows)
//   2. ldband_rank_kernel    per window the exclusive prefix of its masks' popcounts: the rank of every block's first site
//   3. ldband_gather_kernel  one wave per 64-site block: the qualifying rows ANDed with P, their carrier counts and coordinates, each
//                            at its rank                                                                      (streams the rows)
//   4. ldband_pairs_kernel   grid = (window, tile of 256 sites j) items, enumerated exactly from q.  A lane owns site j, its row in
//                            registers up to 32 dwords; the sites j - B .. j + B go through LDS 256 at a time and are read as
//                            broadcasts; a wave skips a staged block that lies wholly outside its lanes' bands.  Every pair is
//                            evaluated from both of its sites: a site's score, partner count, strong count and strong mask stay in
//                            its lane's registers and are stored once, and no per-pair atomic exists.  The pair's record and bin
//                            counters are tallied from its left site alone.  A lane meets its right partners by growing distance, so
//                            it keeps the current bin's counters in registers and flushes them only when the bin changes.
//   5. ldband_prune_kernel   one wave per window: the strong masks staged 64 sites at a time (the next 64 in flight meanwhile),
//                            word w of the kept window in lane w
//   6. ldband_reduce_kernel  one workgroup per window: adds the site rows up, holds them against the pair kernel's totals, writes the record
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "chunk_run.h"
#include "device_utils.h"
#include "internal.h"
#include "ld_select.h"
#include "ldband_math.h"
#include "scan_route.h"
#include "win_chunks.h"

namespace impop {

constexpr uint32_t LB_T = 256;                 // sites of a tile = threads of the pair kernel's workgroup
constexpr size_t LB_LDS_BYTES = 160 * 1024;    // LDS of a CU: what one workgroup of the pair kernel takes at most
constexpr uint32_t PRUNE_U = 8;                // strong masks the prune kernel reads ahead of the kept window's chain

struct LdbandItem {
    uint32_t win, tile;
};

struct LdbandAcc {  // per window of a chunk, zeroed before the chunk's kernels
    uint64_t n_pairs, sum_r2_fx, n_strong, n_perfect;
    uint32_t gathered, n_kept;
};

struct LdbandArgs {
    uint32_t wps, nP, band, sw;            // sw = words of a strong mask
    uint32_t n_bins, thr_num, thr_den;
    uint32_t lds_bins;                     // n_bins where the decay counters live in LDS, else 0
    uint64_t bin_width, max_dist;
};

// the LDS of the pair kernel in front of the decay counters: staged rows | carrier counts | coordinates | four totals
inline size_t ldband_lds_fixed(uint32_t stride) { return ((size_t)LB_T * stride + LB_T) * 4 + (size_t)LB_T * 8 + 4 * 8; }

// grid = windows of the chunk.  rank0[blk_off + i] = qualifying sites of the window in front of its block i; qv[w] = q.
__global__ __launch_bounds__(LD_T) void ldband_rank_kernel(const uint64_t *__restrict__ qmask, const LdWin *__restrict__ wins,
                                                           uint32_t *__restrict__ rank0, uint32_t *__restrict__ qv) {
    __shared__ uint32_t s_scan[LD_T];
    const uint32_t tid = threadIdx.x;
    const LdWin w = wins[blockIdx.x];
    const uint64_t nb = w.s1 > w.s0 ? ((w.s1 + 63) >> 6) - (w.s0 >> 6) : 0;
    const uint64_t *qw = qmask + w.blk_off;
    uint32_t *rk = rank0 + w.blk_off;
    // a thread owns a run of consecutive blocks, as in ld_gather_kernel: its count, one scan over the threads, then its ranks
    const uint64_t seg = (nb + LD_T - 1) / LD_T;
    const uint64_t i_begin = (uint64_t)tid * seg < nb ? (uint64_t)tid * seg : nb, i_end = i_begin + seg < nb ? i_begin + seg : nb;
    uint32_t mine = 0;
    for (uint64_t i = i_begin; i < i_end; ++i) mine += (uint32_t)__popcll(qw[i]);
    s_scan[tid] = mine;
    __syncthreads();
    for (uint32_t off = 1; off < LD_T; off <<= 1) {
        const uint32_t v = tid >= off ? s_scan[tid - off] : 0u;
        __syncthreads();
        s_scan[tid] += v;
        __syncthreads();
    }
    uint32_t rank = s_scan[tid] - mine;
    for (uint64_t i = i_begin; i < i_end; ++i) {
        rk[i] = rank;
        rank += (uint32_t)__popcll(qw[i]);
    }
    if (tid == 0) qv[blockIdx.x] = s_scan[LD_T - 1];
}

// grid = (windows of the chunk, slices of a window's blocks), one wave per 64-site block as in ld_select_kernel.  A window's slots
// number w.cap = its q as the counting pass found it; nothing is written past them, and acc[w].gathered counts what was written.
__global__ __launch_bounds__(LD_T) void ldband_gather_kernel(const uint32_t *__restrict__ sb, const LdWin *__restrict__ wins, uint32_t wps,
                                                             uint32_t G, uint32_t r, const uint32_t *__restrict__ pbits,
                                                             const uint64_t *__restrict__ pos, const uint64_t *__restrict__ qmask,
                                                             const uint32_t *__restrict__ rank0, uint32_t *__restrict__ rows,
                                                             uint32_t *__restrict__ cs, uint64_t *__restrict__ coords,
                                                             LdbandAcc *__restrict__ acc) {
    const uint32_t lane = threadIdx.x & 63, wave = (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const LdWin w = wins[blockIdx.x];
    if (w.s1 <= w.s0) return;
    const uint64_t b0 = w.s0 >> 6, b1 = (w.s1 + 63) >> 6;
    for (uint64_t b = b0 + (uint64_t)blockIdx.y * 4 + wave; b < b1; b += 4ull * gridDim.y) {
        const uint64_t mask = qmask[w.blk_off + (b - b0)];
        if (!mask) continue;  // the whole wave
        const uint32_t rank = rank0[w.blk_off + (b - b0)] + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        const bool take = ((mask >> lane) & 1ull) && rank < w.cap;
        const uint64_t slot = w.row_off + (take ? rank : 0u);
        uint32_t *dst = rows + slot * wps;
        uint32_t c = 0;
        sb_for_each_dword<true>(sb + b * 64ull * wps, G, r, lane, [&](uint32_t k, uint32_t d) {
            const uint32_t v = d & pbits[k];
            c += __popc(v);
            if (take) dst[k] = v;
        });
        if (take) {
            const uint64_t site = b * 64 + lane;
            cs[slot] = c;
            coords[slot] = pos ? pos[site] : site;
        }
        const uint64_t taken = __ballot(take);
        if (lane == 0) atomicAdd(&acc[blockIdx.x].gathered, (uint32_t)__popcll(taken));
    }
}

// WR > 0: a row has at most WR dwords and is kept in registers, LDS rows are padded to WR with zeros; WR == 0: any wps, the
// lane's own row is read from the scratch.  Staged rows are only ever read at one address by the whole wave (a broadcast: no
// bank conflict at any stride) and written with consecutive addresses, so the rows need no padding.
// Dynamic LDS: LB_T rows of (WR ? WR : wps) dwords | LB_T carrier counts | LB_T coordinates | 4 totals | 3 lds_bins counters.
template <uint32_t WR>
__global__ __launch_bounds__(LB_T) void ldband_pairs_kernel(const uint32_t *__restrict__ rows, const uint32_t *__restrict__ cs,
                                                            const uint64_t *__restrict__ coords, const LdWin *__restrict__ wins,
                                                            const LdbandItem *__restrict__ items, const LdbandArgs a,
                                                            uint64_t *__restrict__ strongmask, impop_ldband_site *__restrict__ tab,
                                                            LdbandAcc *__restrict__ acc, unsigned long long *__restrict__ bins) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lb_lds[];
    const LdbandItem it = items[blockIdx.x];
    const LdWin w = wins[it.win];
    const uint32_t m = w.cap, j0 = it.tile * LB_T, tid = threadIdx.x;
    if (j0 >= m) return;  // the whole workgroup: the one item of a chunk whose windows hold no qualifying site
    const uint32_t *grow = rows + w.row_off * a.wps, *gcs = cs + w.row_off;
    const uint64_t *gcoord = coords + w.row_off;
    const uint32_t stride = WR ? WR : a.wps;
    uint32_t *lrow = lb_lds, *lc = lb_lds + LB_T * stride;
    uint64_t *lcoord = reinterpret_cast<uint64_t *>(lc + LB_T);
    unsigned long long *ltot = reinterpret_cast<unsigned long long *>(lcoord + LB_T), *lbin = ltot + 4;
    unsigned long long *gbin = bins ? bins + (uint64_t)it.win * 3ull * a.n_bins : nullptr;
    if (tid < 4) ltot[tid] = 0ull;
    for (uint32_t i = tid; i < 3u * a.lds_bins; i += LB_T) lbin[i] = 0ull;  // the first barrier below orders these

    const uint32_t j = j0 + tid;
    const bool live = j < m;
    uint32_t mine[WR ? WR : 1];
    if (WR) {
#pragma unroll
        for (uint32_t u = 0; u < WR; ++u) mine[u] = live && u < a.wps ? grow[(uint64_t)j * a.wps + u] : 0u;
    }
    const uint32_t *own = grow + (uint64_t)(live ? j : 0u) * a.wps;
    const uint32_t cj = live ? gcs[j] : 0u;
    const uint64_t coordj = live ? gcoord[j] : 0ull;
    const int64_t n = a.nP, vj = (int64_t)cj * (int64_t)(a.nP - cj);
    uint64_t *smj = strongmask + (w.row_off + (live ? j : 0u)) * a.sw;
    const uint32_t reach = j < a.band ? j : a.band;  // the offsets 1..reach lie inside the window
    if (live)
        for (uint32_t wd = ldband_words(reach); wd < a.sw; ++wd) smj[wd] = 0ull;  // the words the walk below never closes

    uint64_t score = 0, cur = 0, t_pairs = 0, t_fx = 0, t_strong = 0, t_perfect = 0, b_fx = 0;
    uint32_t partners = 0, n_strong = 0, b_bin = 0, b_pairs = 0, b_strong = 0;
    auto flush_bin = [&]() {
        if (!b_pairs) return;
        unsigned long long *dst = (a.lds_bins ? lbin : gbin) + 3u * b_bin;
        atomicAdd(dst, (unsigned long long)b_pairs);
        atomicAdd(dst + 1, (unsigned long long)b_fx);
        if (b_strong) atomicAdd(dst + 2, (unsigned long long)b_strong);
        b_pairs = b_strong = 0;
        b_fx = 0;
    };

    // the wave's sites and the partners any of them has
    const uint32_t ja = j0 + (tid & ~63u), jb = ja + 63u < m ? ja + 63u : m - 1u;
    const uint32_t wave_lo = ja > a.band ? ja - a.band : 0u, wave_hi = jb + a.band + 1u < m ? jb + a.band + 1u : m;  // [lo, hi)
    const uint32_t first = (j0 > a.band ? j0 - a.band : 0u) & ~(LB_T - 1u);
    const uint32_t last = j0 + LB_T - 1u + a.band < m - 1u ? j0 + LB_T - 1u + a.band : m - 1u;
    for (uint32_t k0 = first; k0 <= last; k0 += LB_T) {
        const uint32_t kn = m - k0 < LB_T ? m - k0 : LB_T;
        __syncthreads();  // the block before this one has been read
        for (uint32_t idx = tid; idx < kn * stride; idx += LB_T) {
            const uint32_t k = idx / stride, u = idx % stride;
            lrow[idx] = u < a.wps ? grow[(uint64_t)(k0 + k) * a.wps + u] : 0u;
        }
        if (tid < kn) {
            lc[tid] = gcs[k0 + tid];
            lcoord[tid] = gcoord[k0 + tid];
        }
        __syncthreads();
        if (ja >= m) continue;  // a wave without a site
        const uint32_t lo = wave_lo > k0 ? wave_lo : k0, hi = wave_hi < k0 + kn ? wave_hi : k0 + kn;
        for (uint32_t k = lo; k < hi; ++k) {  // wave-uniform: every LDS read below is a broadcast
            const uint32_t kk = k - k0;
            const bool left = k < j;
            const uint32_t off = left ? j - k : k - j;
            if (!live || off == 0u || off > a.band) continue;
            const uint64_t ck64 = lcoord[kk], d = left ? coordj - ck64 : ck64 - coordj;
            if (a.max_dist == 0ull || d <= a.max_dist) {
                uint32_t n11 = 0;
                if (WR) {
#pragma unroll
                    for (uint32_t u = 0; u < WR; ++u) n11 += __popc(mine[u] & lrow[kk * WR + u]);
                } else {
                    for (uint32_t u = 0; u < a.wps; ++u) n11 += __popc(own[u] & lrow[kk * stride + u]);
                }
                const uint32_t ck = lc[kk];
                const int64_t num = n * (int64_t)n11 - (int64_t)cj * (int64_t)ck;
                const int64_t den = vj * ((int64_t)ck * (int64_t)(a.nP - ck));
                const uint64_t fx = ldband_fx(num, den);
                const bool strong = ldband_strong(num, den, a.thr_num, a.thr_den);
                score += fx;
                ++partners;
                n_strong += strong;
                if (left) {
                    if (strong) cur |= 1ull << ((off - 1u) & 63u);
                } else {
                    ++t_pairs;
                    t_fx += fx;
                    t_strong += strong;
                    t_perfect += ldband_perfect(num, den);
                    if (gbin) {
                        const uint32_t bin = ldband_bin(d, a.bin_width, a.n_bins);
                        if (bin != b_bin) {
                            flush_bin();
                            b_bin = bin;
                        }
                        ++b_pairs;
                        b_fx += fx;
                        b_strong += strong;
                    }
                }
            }
            if (left && ((off - 1u) & 63u) == 0u) {  // the lowest bit of a word of the strong mask: the word is complete
                smj[(off - 1u) >> 6] = cur;
                cur = 0ull;
            }
        }
    }
    flush_bin();
    if (t_pairs) {
        atomicAdd(&ltot[0], (unsigned long long)t_pairs);
        atomicAdd(&ltot[1], (unsigned long long)t_fx);
        if (t_strong) atomicAdd(&ltot[2], (unsigned long long)t_strong);
        if (t_perfect) atomicAdd(&ltot[3], (unsigned long long)t_perfect);
    }
    if (live) {
        impop_ldband_site out;
        out.coord = coordj;
        out.ld_score_fx = score;
        out.carriers = cj;
        out.n_partners = partners;
        out.n_strong = n_strong;
        out.kept = 0u;  // the prune kernel's
        tab[w.row_off + j] = out;
    }
    __syncthreads();
    if (tid < 4 && ltot[tid]) atomicAdd(reinterpret_cast<unsigned long long *>(&acc[it.win].n_pairs) + tid, ltot[tid]);
    for (uint32_t i = tid; i < 3u * a.lds_bins; i += LB_T)
        if (lbin[i]) atomicAdd(gbin + i, lbin[i]);
}

// grid = windows of the chunk, one wave each: lane w < sw holds word w of the kept window
__global__ __launch_bounds__(64) void ldband_prune_kernel(const uint64_t *__restrict__ strongmask, const LdWin *__restrict__ wins, uint32_t sw,
                                                          impop_ldband_site *__restrict__ tab, LdbandAcc *__restrict__ acc) {
    __shared__ uint64_t buf[64 * LDBAND_MAX_WORDS];
    const uint32_t lane = threadIdx.x;
    const LdWin w = wins[blockIdx.x];
    const uint32_t m = w.cap;
    const uint64_t *sm = strongmask + w.row_off * sw;
    uint64_t K = 0ull;
    uint32_t n_kept = 0;
    // the masks of the NEXT 64 sites are loaded into registers while the chain runs over the staged ones: entry lane + 64 i
    uint64_t pre[LDBAND_MAX_WORDS];
    auto fetch = [&](uint32_t j0) {
        const uint32_t entries = j0 < m ? (m - j0 < 64u ? m - j0 : 64u) * sw : 0u;
#pragma unroll
        for (uint32_t i = 0; i < LDBAND_MAX_WORDS; ++i) pre[i] = lane + 64u * i < entries ? sm[(uint64_t)j0 * sw + lane + 64u * i] : 0ull;
    };
    fetch(0u);
    for (uint32_t j0 = 0; j0 < m; j0 += 64) {
        const uint32_t cnt = m - j0 < 64u ? m - j0 : 64u;
        __syncthreads();  // the block before this one has been read
#pragma unroll
        for (uint32_t i = 0; i < LDBAND_MAX_WORDS; ++i)
            if (lane + 64u * i < cnt * sw) buf[lane + 64u * i] = pre[i];
        __syncthreads();
        fetch(j0 + 64u);
        uint64_t keptmask = 0ull;
        // the chain from one site to the next is K alone: the masks of PRUNE_U sites are read ahead of it, and the carry moves
        // one lane up by a DPP row shift (sw <= 16: the words live in the first row of 16 lanes), not through LDS
        for (uint32_t t0 = 0; t0 < cnt; t0 += PRUNE_U) {
            uint64_t S[PRUNE_U];
#pragma unroll
            for (uint32_t u = 0; u < PRUNE_U; ++u) S[u] = lane < sw && t0 + u < cnt ? buf[(t0 + u) * sw + lane] : 0ull;
#pragma unroll
            for (uint32_t u = 0; u < PRUNE_U; ++u) {
                if (t0 + u >= cnt) break;  // the whole wave
                const bool kept = __ballot(ldband_word_hit(K, S[u])) == 0ull;
                uint32_t carry = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)ldband_word_carry(K), 0x111 /* row_shr:1 */, 0xF, 0xF, false);
                if (lane == 0) carry = kept ? 1u : 0u;
                K = lane < sw ? ldband_word_shift(K, (uint64_t)carry) : 0ull;
                keptmask |= (uint64_t)kept << (t0 + u);
            }
        }
        if (lane < cnt) tab[w.row_off + j0 + lane].kept = (uint32_t)((keptmask >> lane) & 1ull);
        n_kept += (uint32_t)__popcll(keptmask);
    }
    if (lane == 0) acc[blockIdx.x].n_kept = n_kept;
}

// grid = windows of the chunk, one workgroup each (after the prune kernel: it reads kept)
__global__ __launch_bounds__(LB_T) void ldband_reduce_kernel(const impop_ldband_site *__restrict__ tab, const LdWin *__restrict__ wins,
                                                           const uint32_t *__restrict__ qv, const LdbandAcc *__restrict__ acc,
                                                           const unsigned long long *__restrict__ bins, uint32_t n_bins, uint32_t nP,
                                                           impop_ldband_stats *__restrict__ rec, uint32_t *__restrict__ err) {
    __shared__ unsigned long long s[5];
    const uint32_t lane = threadIdx.x, win = blockIdx.x;
    const LdWin w = wins[win];
    const uint32_t m = w.cap;
    if (lane < 5) s[lane] = 0ull;
    __syncthreads();
    unsigned long long partners = 0, score = 0, strong = 0, kept = 0, bin_pairs = 0;
    for (uint32_t j = lane; j < m; j += LB_T) {
        const impop_ldband_site row = tab[w.row_off + j];
        partners += row.n_partners;
        score += row.ld_score_fx;
        strong += row.n_strong;
        kept += row.kept;
    }
    if (bins)
        for (uint32_t b = lane; b < n_bins; b += LB_T) bin_pairs += bins[((uint64_t)win * n_bins + b) * 3ull];
    atomicAdd(&s[0], partners);
    atomicAdd(&s[1], score);
    atomicAdd(&s[2], strong);
    atomicAdd(&s[3], kept);
    atomicAdd(&s[4], bin_pairs);
    __syncthreads();
    if (lane != 0) return;
    const LdbandAcc a = acc[win];
    const bool first_kept = m == 0u || tab[w.row_off].kept == 1u;
    if (qv[win] != m || a.gathered != m || a.n_kept > m || s[3] != a.n_kept || !first_kept || s[0] != 2ull * a.n_pairs ||
        s[1] != 2ull * a.sum_r2_fx || s[2] != 2ull * a.n_strong || (bins && s[4] != a.n_pairs))
        atomicOr(err, DEV_ERR_LDBAND);
    impop_ldband_stats out;
    out.n_members = nP;
    out.n_sites = w.n_sites;
    out.n_qualifying = qv[win];
    out.n_kept = a.n_kept;
    out.n_pairs = a.n_pairs;
    out.sum_r2_fx = a.sum_r2_fx;
    out.n_strong = a.n_strong;
    out.n_perfect = a.n_perfect;
    out.site_off = 0ull;  // the host's: the prefix over all windows of the call
    out.mean_r2 = 0.0;    // the host's, from the integers
    rec[win] = out;
}

template <uint32_t WR>
static int launch_ldband_pairs(impop_ctx *ctx, uint32_t n_items, size_t lds, const uint32_t *rows, const uint32_t *cs, const uint64_t *coords,
                               const LdWin *wins, const LdbandItem *items, const LdbandArgs &a, uint64_t *sm, impop_ldband_site *tab,
                               LdbandAcc *acc, unsigned long long *bins) {
    const int rc = lds_opt_in(ldband_pairs_kernel<WR>, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(ldband_pairs_kernel<WR>, dim3(n_items), dim3(LB_T), lds, ctx->stream, rows, cs, coords, wins, items, a, sm, tab, acc,
                       bins);
    return IMPOP_OK;
}

}  // namespace impop

using namespace impop;

static_assert(IMPOP_LDBAND_MAX_N == LDBAND_MAX_N && IMPOP_LDBAND_MAX_BAND == LDBAND_MAX_BAND && IMPOP_LDBAND_MAX_BINS == LDBAND_MAX_BINS &&
              IMPOP_LDBAND_FX_ONE == LDBAND_FX_ONE, "the header's constants");

IMPOP_API int impop_ldband_scan(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows,
                                const uint64_t *mask_p, const impop_ldband_params *params, impop_ldband_stats *out_host,
                                impop_ldband_bin *bins, impop_ldband_site *site_table, uint64_t site_capacity, uint64_t *n_site_rows) {
    static_assert(sizeof(impop_ldband_stats) == 64 && sizeof(impop_ldband_params) == 48 && sizeof(impop_ldband_site) == 32 &&
                  sizeof(impop_ldband_bin) == 24 && sizeof(LdbandItem) == 8 && sizeof(LdbandAcc) == 40, "ABI layout");
    const char *fn = "impop_ldband_scan";
    REQUIRE(ctx && m && params, "%s: NULL argument", fn);
    REQUIRE(params->struct_size == sizeof(impop_ldband_params), "impop_ldband_params.struct_size mismatch");
    REQUIRE(m->device == ctx->device, "%s: matrix lives on device %d, context on %d", fn, m->device, ctx->device);
    const uint32_t n = m->g.n_hap, wps = m->g.wps;
    const MemberSet P = member_set(mask_p, n, wps);
    const uint32_t nP = P.size();
    REQUIRE(nP > 0, "%s: the mask selects no haplotype", fn);
    REQUIRE(params->min_mac >= 1, "%s: min_mac must be at least 1", fn);
    const uint32_t band = params->band_sites, n_bins = params->n_bins, sw = ldband_words(band);
    REQUIRE(band >= 1 && band <= IMPOP_LDBAND_MAX_BAND, "%s: band_sites %u outside 1..%u", fn, band, (uint32_t)IMPOP_LDBAND_MAX_BAND);
    REQUIRE(n_bins >= 1 && n_bins <= IMPOP_LDBAND_MAX_BINS, "%s: n_bins %u outside 1..%u", fn, n_bins, (uint32_t)IMPOP_LDBAND_MAX_BINS);
    REQUIRE(params->bin_width >= 1, "%s: bin_width must be at least 1", fn);
    REQUIRE(params->thr_den >= 1 && params->thr_den <= 65535u && params->thr_num <= params->thr_den,
            "%s: threshold %u/%u: thr_den must be 1..65535 and thr_num at most thr_den", fn, params->thr_num, params->thr_den);
    int rc = check_windows(fn, m, windows, windows ? n_windows : 0);
    if (rc) return rc;
    if (nP > IMPOP_LDBAND_MAX_N) {
        set_error("%s: %u members exceed the limit (%u)", fn, nP, (uint32_t)IMPOP_LDBAND_MAX_N);
        return IMPOP_E_UNSUPPORTED;
    }
    if (!n_windows) {
        if (n_site_rows) *n_site_rows = 0;
        return IMPOP_OK;
    }
    REQUIRE(windows && out_host, "%s: NULL windows/out", fn);
    std::vector<impop_window> mapped;
    map_windows(m, windows, n_windows, mapped);
    if ((rc = check_window_weights(fn, m, windows, n_windows))) return rc;

    const uint64_t budget = chunk_budget(params->max_chunk_bytes);
    std::vector<uint64_t> nb(n_windows);  // the 64-site blocks a window touches
    uint64_t block_bytes = 0;
    for (uint64_t i = 0; i < n_windows; ++i) {
        nb[i] = ld_blocks(mapped[i].site_begin, mapped[i].site_end);
        block_bytes += nb[i] * 256ull * wps;
    }
    auto fill_wins = [&](const WinChunk &c, LdWin *h_wins, const uint32_t *q, uint64_t *longest) {
        uint64_t n_blocks = 0, n_slots = 0;
        *longest = 0;
        for (uint64_t i = c.w_begin; i < c.w_end; ++i) {
            h_wins[i - c.w_begin] = LdWin{mapped[i].site_begin, mapped[i].site_end, n_blocks, n_slots,
                                          (uint32_t)window_W(m, windows[i].site_begin, windows[i].site_end), q ? q[i] : 0u};
            n_blocks += nb[i];
            n_slots += q ? q[i] : 0u;
            *longest = std::max(*longest, nb[i]);
        }
    };
    auto select = [&](const ChunkRun &run, EventPairs &T, size_t cnt, uint64_t longest, const LdWin *d_wins, const uint32_t *d_pbits,
                      uint64_t *d_qmask) {
        return run.timed(T, [&] {
            hipLaunchKernelGGL(ld_select_kernel, dim3((uint32_t)cnt, ld_select_slices(longest)), dim3(LD_T), 0, ctx->stream, m->d_sb, d_wins,
                               wps, m->g.G, m->g.r, d_pbits, nP, params->min_mac, d_qmask);
        });
    };
    HIP_TRY(hipSetDevice(ctx->device));
    EventPairs *timer = ctx->timers + impop_ctx::T_LDBAND;
    uint64_t launches = 0;

    // ---- count: q of every window, before anything is written
    std::vector<uint32_t> q(n_windows);
    {
        const std::vector<WinChunk> chunks =
            cut_windows(n_windows, budget, 0, [&](size_t, uint64_t i) { return sizeof(LdWin) + 4 + nb[i] * 12; });
        const size_t max_wins = max_over(chunks, [](const WinChunk &c) { return c.w_end - c.w_begin; });
        const size_t max_blocks = max_over(chunks, [&](const WinChunk &c) {
            uint64_t sum = 0;
            for (uint64_t i = c.w_begin; i < c.w_end; ++i) sum += nb[i];
            return sum;
        });
        REQUIRE(max_wins < 0x7FFFFFFFull, "%s: a chunk of %zu windows exceeds one launch", fn, max_wins);
        Carve L;
        const size_t o_pbits = L.take<uint32_t>(wps), o_wins = L.take<LdWin>(max_wins), o_qv = L.take<uint32_t>(max_wins), staged = L.total(),
                     o_qmask = L.take<uint64_t>(max_blocks), o_rank = L.take<uint32_t>(max_blocks);
        void *d = nullptr, *pin = nullptr;
        if ((rc = ctx_scratch(ctx, L.total(), &d))) return rc;
        if ((rc = ctx_pinned(ctx, staged, &pin))) return rc;
        const ChunkRun run{ctx, fn, (char *)d, (char *)pin};
        memcpy(run.hc + o_pbits, P.bits.data(), (size_t)wps * 4);
        if ((rc = run.up(o_pbits, o_pbits + (size_t)wps * 4))) return rc;
        for (const WinChunk &c : chunks) {
            const size_t cnt = c.w_end - c.w_begin;
            uint64_t longest = 0;
            fill_wins(c, (LdWin *)(run.hc + o_wins), nullptr, &longest);
            if ((rc = run.up(o_wins, o_wins + cnt * sizeof(LdWin)))) return rc;
            if ((rc = select(run, timer[0], cnt, longest, (const LdWin *)(run.dc + o_wins), (const uint32_t *)(run.dc + o_pbits),
                             (uint64_t *)(run.dc + o_qmask)))) return rc;
            if ((rc = run.timed(timer[1], [&] {
                hipLaunchKernelGGL(ldband_rank_kernel, dim3((uint32_t)cnt), dim3(LD_T), 0, ctx->stream, (const uint64_t *)(run.dc + o_qmask),
                                   (const LdWin *)(run.dc + o_wins), (uint32_t *)(run.dc + o_rank), (uint32_t *)(run.dc + o_qv));
            }))) return rc;
            launches += 2;
            if ((rc = run.finish(o_qv, o_qv + cnt * 4))) return rc;
            memcpy(q.data() + c.w_begin, run.hc + o_qv, cnt * 4);
        }
    }
    // the one refusal that needs q
    const uint64_t slot_core = 4ull * wps + 8ull * sw + sizeof(impop_ldband_site);
    uint64_t total = 0;
    for (uint64_t i = 0; i < n_windows; ++i) {
        if ((uint64_t)q[i] * slot_core > budget || (uint64_t)q[i] * band >= (1ull << 34)) {
            set_error("%s: window %llu has %u qualifying sites: %llu bytes of rows, strong masks and site rows against max_chunk_bytes "
                      "%llu, %llu site x band slots against 2^34", fn, (unsigned long long)i, q[i],
                      (unsigned long long)(q[i] * slot_core), (unsigned long long)budget, (unsigned long long)((uint64_t)q[i] * band));
            return IMPOP_E_UNSUPPORTED;
        }
        total += q[i];
    }
    if (n_site_rows) *n_site_rows = total;
    const bool want_table = site_table && site_capacity >= total;

    // ---- work: chunks cut from the real q
    // a slot's device bytes: the gathered row, its c, its coordinate, its strong mask, its site row; a window's: the record, the
    // descriptor, q, the accumulators, its decay counters, a mask and a rank per block, an item per tile of its slots
    const uint64_t per_slot = slot_core + 4 + 8;
    const uint64_t per_win = sizeof(impop_ldband_stats) + sizeof(LdWin) + 4 + sizeof(LdbandAcc) + (bins ? (uint64_t)n_bins * 24 : 0);
    auto tiles_of = [](uint64_t sites) { return (sites + LB_T - 1) / LB_T; };
    const std::vector<WinChunk> chunks = cut_windows(n_windows, budget, 0, [&](size_t, uint64_t i) {
        return per_win + nb[i] * 12 + q[i] * per_slot + tiles_of(q[i]) * sizeof(LdbandItem);
    });
    auto chunk_sum = [&](auto f) {
        return max_over(chunks, [&](const WinChunk &c) {
            uint64_t sum = 0;
            for (uint64_t i = c.w_begin; i < c.w_end; ++i) sum += f(i);
            return sum;
        });
    };
    const size_t max_wins = max_over(chunks, [](const WinChunk &c) { return c.w_end - c.w_begin; });
    const size_t max_blocks = chunk_sum([&](uint64_t i) { return nb[i]; }), max_slots = chunk_sum([&](uint64_t i) { return (uint64_t)q[i]; });
    const size_t max_items = chunk_sum([&](uint64_t i) { return tiles_of(q[i]); });
    REQUIRE(max_wins < 0x7FFFFFFFull && max_items < 0x7FFFFFFFull, "%s: a chunk of %zu windows exceeds one launch", fn, max_wins);

    // device: P as dwords | windows, items (up, through the page-locked staging with the same offsets) | records (down, staged) |
    // q, accumulators, decay counters | qualifying masks, block ranks | gathered rows, their c, coordinates, strong masks, site rows
    Carve L;
    const size_t o_pbits = L.take<uint32_t>(wps), o_wins = L.take<LdWin>(max_wins), o_items = L.take<LdbandItem>(max_items),
                 o_rec = L.take<impop_ldband_stats>(max_wins), staged = L.total(), o_qv = L.take<uint32_t>(max_wins),
                 o_acc = L.take<LdbandAcc>(max_wins), o_bins = L.take<impop_ldband_bin>(bins ? max_wins * n_bins : 0),
                 o_qmask = L.take<uint64_t>(max_blocks), o_rank = L.take<uint32_t>(max_blocks), o_rows = L.take<uint32_t>(max_slots * wps),
                 o_cs = L.take<uint32_t>(max_slots), o_coords = L.take<uint64_t>(max_slots), o_sm = L.take<uint64_t>(max_slots * sw),
                 o_tab = L.take<impop_ldband_site>(max_slots);
    void *d = nullptr, *pin = nullptr;
    if ((rc = ctx_scratch(ctx, L.total(), &d))) return rc;
    if ((rc = ctx_pinned(ctx, staged, &pin))) return rc;
    const ChunkRun run{ctx, fn, (char *)d, (char *)pin};
    char *dc = run.dc, *hc = run.hc;
    memcpy(hc + o_pbits, P.bits.data(), (size_t)wps * 4);
    if ((rc = run.up(o_pbits, o_pbits + (size_t)wps * 4))) return rc;

    const uint32_t WR = wps <= 4 ? 4u : wps <= 8 ? 8u : wps <= 16 ? 16u : wps <= 32 ? 32u : 0u;
    // the decay counters in LDS where they fit beside the staged rows; IMPOP_LDBAND_LDS_BINS=n lowers what the LDS form takes, so
    // that tests reach the global form at small sizes
    const size_t lds_fixed = ldband_lds_fixed(WR ? WR : wps);
    size_t lds_cap = lds_fixed < LB_LDS_BYTES ? (LB_LDS_BYTES - lds_fixed) / 24 : 0;
    if (const char *e = getenv("IMPOP_LDBAND_LDS_BINS"); e && *e) {
        const long v = strtol(e, nullptr, 10);
        lds_cap = std::min<size_t>(lds_cap, v < 0 ? 0 : (size_t)v);
    }
    const bool lds_bins = bins && n_bins <= lds_cap;
    const size_t lds_pairs = lds_fixed + (lds_bins ? (size_t)n_bins * 24 : 0);
    REQUIRE(lds_pairs <= LB_LDS_BYTES, "%s: %zu bytes of LDS for rows of %u dwords", fn, lds_pairs, wps);
    const LdbandArgs args{wps, nP, band, sw, n_bins, params->thr_num, params->thr_den, lds_bins ? n_bins : 0u, params->bin_width,
                          params->max_dist};

    const uint32_t *d_pbits = (const uint32_t *)(dc + o_pbits);
    const LdWin *d_wins = (const LdWin *)(dc + o_wins);
    const LdbandItem *d_items = (const LdbandItem *)(dc + o_items);
    impop_ldband_stats *d_rec = (impop_ldband_stats *)(dc + o_rec);
    uint32_t *d_qv = (uint32_t *)(dc + o_qv), *d_rank = (uint32_t *)(dc + o_rank), *d_rows = (uint32_t *)(dc + o_rows),
             *d_cs = (uint32_t *)(dc + o_cs);
    LdbandAcc *d_acc = (LdbandAcc *)(dc + o_acc);
    unsigned long long *d_bins = bins ? (unsigned long long *)(dc + o_bins) : nullptr;
    uint64_t *d_qmask = (uint64_t *)(dc + o_qmask), *d_coords = (uint64_t *)(dc + o_coords), *d_sm = (uint64_t *)(dc + o_sm);
    impop_ldband_site *d_tab = (impop_ldband_site *)(dc + o_tab);
    LdWin *h_wins = (LdWin *)(hc + o_wins);
    LdbandItem *h_items = (LdbandItem *)(hc + o_items);
    uint64_t qualifying = 0, pairs = 0, site_off = 0;
    for (const WinChunk &c : chunks) {
        const size_t cnt = c.w_end - c.w_begin;
        uint64_t longest = 0, n_slots = 0;
        uint32_t n_items = 0;
        fill_wins(c, h_wins, q.data(), &longest);
        for (size_t k = 0; k < cnt; ++k) {
            n_slots += q[c.w_begin + k];
            for (uint32_t t = 0; t < tiles_of(q[c.w_begin + k]); ++t) h_items[n_items++] = LdbandItem{(uint32_t)k, t};
        }
        if (!n_items) h_items[n_items++] = LdbandItem{0u, 0u};  // windows without qualifying sites only: the one item leaves at once
        if ((rc = run.up(o_wins, o_items + n_items * sizeof(LdbandItem)))) return rc;
        HIP_TRY(hipMemsetAsync(d_acc, 0, cnt * sizeof(LdbandAcc), ctx->stream));
        if (bins) HIP_TRY(hipMemsetAsync(d_bins, 0, cnt * (size_t)n_bins * 24, ctx->stream));
        if ((rc = select(run, timer[0], cnt, longest, d_wins, d_pbits, d_qmask))) return rc;
        if ((rc = run.timed(timer[1], [&] {
            hipLaunchKernelGGL(ldband_rank_kernel, dim3((uint32_t)cnt), dim3(LD_T), 0, ctx->stream, d_qmask, d_wins, d_rank, d_qv);
            hipLaunchKernelGGL(ldband_gather_kernel, dim3((uint32_t)cnt, ld_select_slices(longest)), dim3(LD_T), 0, ctx->stream, m->d_sb,
                               d_wins, wps, m->g.G, m->g.r, d_pbits, m->compact ? m->d_pos : nullptr, d_qmask, d_rank, d_rows, d_cs,
                               d_coords, d_acc);
        }))) return rc;
        if ((rc = run.timed(timer[2], [&] {
            switch (WR) {
            case 4: return launch_ldband_pairs<4>(ctx, n_items, lds_pairs, d_rows, d_cs, d_coords, d_wins, d_items, args, d_sm, d_tab, d_acc, d_bins);
            case 8: return launch_ldband_pairs<8>(ctx, n_items, lds_pairs, d_rows, d_cs, d_coords, d_wins, d_items, args, d_sm, d_tab, d_acc, d_bins);
            case 16: return launch_ldband_pairs<16>(ctx, n_items, lds_pairs, d_rows, d_cs, d_coords, d_wins, d_items, args, d_sm, d_tab, d_acc, d_bins);
            case 32: return launch_ldband_pairs<32>(ctx, n_items, lds_pairs, d_rows, d_cs, d_coords, d_wins, d_items, args, d_sm, d_tab, d_acc, d_bins);
            default: return launch_ldband_pairs<0>(ctx, n_items, lds_pairs, d_rows, d_cs, d_coords, d_wins, d_items, args, d_sm, d_tab, d_acc, d_bins);
            }
        }))) return rc;
        if ((rc = run.timed(timer[3], [&] {
            hipLaunchKernelGGL(ldband_prune_kernel, dim3((uint32_t)cnt), dim3(64), 0, ctx->stream, d_sm, d_wins, sw, d_tab, d_acc);
        }))) return rc;
        if ((rc = run.timed(timer[4], [&] {
            hipLaunchKernelGGL(ldband_reduce_kernel, dim3((uint32_t)cnt), dim3(LB_T), 0, ctx->stream, d_tab, d_wins, d_qv, d_acc, d_bins, n_bins,
                               nP, d_rec, ctx->d_err);
        }))) return rc;
        launches += 6;
        if (want_table && n_slots)
            HIP_TRY(hipMemcpyAsync(site_table + site_off, d_tab, n_slots * sizeof(impop_ldband_site), hipMemcpyDeviceToHost, ctx->stream));
        if (bins) HIP_TRY(hipMemcpyAsync(bins + c.w_begin * n_bins, d_bins, cnt * (size_t)n_bins * 24, hipMemcpyDeviceToHost, ctx->stream));
        if ((rc = run.finish(o_rec, o_rec + cnt * sizeof(impop_ldband_stats)))) return rc;
        const impop_ldband_stats *rv = (const impop_ldband_stats *)(hc + o_rec);
        for (size_t k = 0; k < cnt; ++k) {
            const uint64_t i = c.w_begin + k;
            impop_ldband_stats r = rv[k];
            REQUIRE(r.n_qualifying == q[i], "%s: window %llu counts %u qualifying sites, then %u", fn, (unsigned long long)i, q[i],
                    r.n_qualifying);
            r.site_off = site_off;
            r.mean_r2 = r.n_pairs ? (double)r.sum_r2_fx / ((double)r.n_pairs * 1073741824.0) : NAN;
            out_host[i] = r;
            site_off += q[i];
            qualifying += q[i];
            pairs += r.n_pairs;
        }
    }
    if (trace_on()) {
        fprintf(stderr, "[impop_ldband_scan] route=%s windows=%llu chunks=%llu launches=%llu qualifying=%llu pairs=%llu band=%u bins=%s "
                "bytes_streamed=%llu\n", m->compact ? "compact" : "dense", (unsigned long long)n_windows, (unsigned long long)chunks.size(),
                (unsigned long long)launches, (unsigned long long)qualifying, (unsigned long long)pairs, band,
                !bins ? "off" : lds_bins ? "lds" : "global", (unsigned long long)(3ull * block_bytes + qualifying * 4ull * wps));
        fflush(stderr);
    }
    return IMPOP_OK;
}

IMPOP_API int impop_ctx_ldband_elapsed(impop_ctx *ctx, double kernel_ms[5], uint64_t *chunks) {
    REQUIRE(ctx && kernel_ms, "impop_ctx_ldband_elapsed: NULL argument");
    return ctx_timers_elapsed(ctx, impop_ctx::T_LDBAND, 5, 2, kernel_ms, chunks);
}
