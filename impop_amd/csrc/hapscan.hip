// hapscan.hip — impop_haplotype_scan: the distinct haplotypes of every window (K, H1, H12, H2/H1, haplotype diversity) from
// the stream the headline scan reads, without the hap-major operand and without the Gram.
//
// Two members of P are the same haplotype in a window iff their bits agree at every column.  Monomorphic columns separate
// nobody, so the variable-site index (rare entries + SB64 rows) decides it as well as the dense matrix does.  Per chunk of
// windows, on the tiles of scan_route (shared by overlapping windows exactly as TilePartials are):
//   1. hap_fingerprint_kernel  one workgroup per tile: a 128-bit fingerprint per member of the member's bits in the tile.  Rows:
//                              ballot transpose of every dword column of a 64-site block into per-haplotype 64-site words, each
//                              mixed with its block index; rare entries: a per-entry key for the listed haplotypes (listing the
//                              zeros separates the same pairs).  Everything combines by XOR, in LDS, then one plain store.
//   2. hap_classify_kernel     one workgroup per window: XOR of its tiles' fingerprints, members grouped by fingerprint in an LDS
//                              hash table, representative = smallest member, sizes, (-size, smallest member) ranking, the record.
//   3. hap_verify_kernel       one workgroup per (window, tile): streams the tile again and checks bit(i) == bit(rep(i)) for
//                              every member at every site.  A fingerprint is never trusted: a mismatch flags the window.
//   4. hap_exact_kernel        flagged windows only (a fingerprint collision: in practice never): greedy equality grouping
//                              against the smallest unassigned member, one streaming pass per class, then the same record.
// The doubles of a record are computed on the host from its integers, in one place.  Chunks: win_chunks.h / chunk_run.h.
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "device_utils.h"
#include "hap_words.h"
#include "internal.h"
#include "sb64.h"
#include "scan_route.h"
#include "win_chunks.h"

namespace impop {

constexpr int HAP_T = 256;  // threads of every workgroup here
constexpr uint32_t HAP_NONE = 0xFFFFFFFFu;
static_assert(IMPOP_HAPLOTYPE_MAX_N <= 4096u, "member indices and sizes are packed into 12 / 16 bits");

struct HapWin {  // a window of a chunk: its tiles (chunk-local) and its W
    uint32_t t0, t1;
    uint32_t n_sites, pad;
};
struct HapItem {  // one workgroup of the verify kernel
    uint32_t win, tile;
};

// grid = tiles of the chunk; dynamic LDS: 16 bytes x nP
__global__ __launch_bounds__(HAP_T) void hap_fingerprint_kernel(const uint32_t *__restrict__ sb, const uint64_t *__restrict__ rare,
                                                                const ScanTile *__restrict__ tiles, uint32_t wps, uint32_t G, uint32_t r,
                                                                const int32_t *__restrict__ ppos, const uint32_t *__restrict__ pmask,
                                                                uint32_t n_pad, uint32_t nP, uint64_t *__restrict__ fp) {
    extern __shared__ unsigned long long hap_acc[];  // (lo, hi) per member
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = (uint32_t)__builtin_amdgcn_readfirstlane(tid >> 6);
    for (uint32_t i = tid; i < 2 * nP; i += HAP_T) hap_acc[i] = 0ull;
    __syncthreads();
    const ScanTile t = tiles[blockIdx.x];
    const TileBlocks tb = tile_blocks_of(t);
    const uint64_t b0 = tb.b0, b1 = tb.b1;
    for (uint64_t b = b0 + wave; b < b1; b += 4) {
        const uint64_t ka = mix64(2 * b + 1), kb = mix64(~b);  // the block's keys: equal words of different blocks differ
        hap_block_words(sb + b * 64ull * wps, G, r, lane, hap_edge(t, b), ppos, pmask, [&](uint32_t pp, uint64_t word) {
            atomicXor(&hap_acc[2 * pp], (unsigned long long)mix64(word ^ ka));
            atomicXor(&hap_acc[2 * pp + 1], (unsigned long long)mix64(word * 0x9E3779B97F4A7C15ull + kb));
        });
    }
    for (uint64_t e = t.rare_begin + tid; e < t.rare_end; e += HAP_T) {
        int32_t pp[IMPOP_RARE_MAX];
        hap_rare_members(stream_load(rare + e), ppos, n_pad, pp);
        const uint64_t lo = mix64(0xA24BAED4963EE407ull ^ e), hi = mix64(0x9FB21C651E98DF25ull + e);
#pragma unroll
        for (uint32_t i = 0; i < IMPOP_RARE_MAX; ++i)
            if (pp[i] >= 0) {
                atomicXor(&hap_acc[2 * pp[i]], (unsigned long long)lo);
                atomicXor(&hap_acc[2 * pp[i] + 1], (unsigned long long)hi);
            }
    }
    __syncthreads();
    uint64_t *dst = fp + (uint64_t)blockIdx.x * 2 * nP;
    for (uint32_t i = tid; i < 2 * nP; i += HAP_T) dst[i] = hap_acc[i];
}

// From rep[i] (the smallest member of i's class) to everything a window reports.  LDS scratch: cnt[nP], rank_of[nP],
// sortbuf[2^ceil(log2 K)].  Classes are ordered by one bitonic sort of (nP - size) << 12 | rep.
//   repsz[i] = rep(i) | size(i's class) << 16 (what the verify kernel reads), class_of / sizes as impop_cluster_scan writes them
__device__ inline void hap_emit(const uint32_t *rep, uint32_t *cnt, uint32_t *rank_of, uint32_t *sortbuf, uint32_t nP, uint32_t n_sites,
                                impop_haplotype_stats *__restrict__ rec, uint32_t *__restrict__ repsz, uint32_t *__restrict__ class_of,
                                uint32_t *__restrict__ sizes, uint32_t *__restrict__ err) {
    __shared__ uint32_t s_k, s_single;
    __shared__ unsigned long long s_sq, s_sum;
    const uint32_t tid = threadIdx.x;
    __syncthreads();
    for (uint32_t i = tid; i < nP; i += HAP_T) cnt[i] = 0;
    if (tid == 0) {
        s_k = 0;
        s_single = 0;
        s_sq = 0;
        s_sum = 0;
    }
    __syncthreads();
    for (uint32_t i = tid; i < nP; i += HAP_T) atomicAdd(&cnt[rep[i]], 1u);
    __syncthreads();
    for (uint32_t i = tid; i < nP; i += HAP_T)
        if (rep[i] == i) sortbuf[atomicAdd(&s_k, 1u)] = ((nP - cnt[i]) << 12) | i;
    __syncthreads();
    const uint32_t K = s_k;
    uint32_t P2 = 1;
    while (P2 < K) P2 <<= 1;
    for (uint32_t j = K + tid; j < P2; j += HAP_T) sortbuf[j] = HAP_NONE;
    __syncthreads();
    for (uint32_t k = 2; k <= P2; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t a = tid; a < P2; a += HAP_T) {
                const uint32_t b = a ^ j;
                if (b > a) {
                    const uint32_t va = sortbuf[a], vb = sortbuf[b];
                    if ((va > vb) == ((a & k) == 0)) {
                        sortbuf[a] = vb;
                        sortbuf[b] = va;
                    }
                }
            }
            __syncthreads();
        }
    uint32_t single = 0;
    unsigned long long sq = 0, sum = 0;
    for (uint32_t j = tid; j < nP; j += HAP_T) {
        uint32_t sz = 0;
        if (j < K) {
            const uint32_t key = sortbuf[j];
            sz = nP - (key >> 12);
            rank_of[key & 0xFFFu] = j;
            single += sz == 1;
            sq += (unsigned long long)sz * sz;
            sum += sz;
        }
        if (sizes) sizes[j] = sz;
    }
    if (single) atomicAdd(&s_single, single);
    if (sq) atomicAdd(&s_sq, sq);
    if (sum) atomicAdd(&s_sum, sum);
    __syncthreads();
    for (uint32_t i = tid; i < nP; i += HAP_T) {
        const uint32_t rp = rep[i];
        repsz[i] = rp | (cnt[rp] << 16);
        if (class_of) class_of[i] = rank_of[rp];
    }
    if (tid == 0) {
        impop_haplotype_stats o;
        o.n_members = nP;
        o.n_distinct = K;
        o.largest = nP - (sortbuf[0] >> 12);
        o.second = K > 1 ? nP - (sortbuf[1] >> 12) : 0u;
        o.n_singletons = s_single;
        o.n_sites = n_sites;
        o.sum_sq = s_sq;
        o.h1 = o.h12 = o.h2_h1 = o.hap_diversity = 0.0;  // the host fills them in from the integers
        *rec = o;
        if (s_sum != nP || K == 0 || K > nP) atomicOr(err, DEV_ERR_HAPSCAN);  // the classes do not partition P
    }
}

// grid = windows of the chunk.  Dynamic LDS: key 16 nP | slot 4 nP | tab 4 T | smin 4 T, T = hash slots (a power of two >= 2 nP);
// once every member knows its slot the key region is hap_emit's scratch.
__global__ __launch_bounds__(HAP_T) void hap_classify_kernel(const uint64_t *__restrict__ fp, const HapWin *__restrict__ wins, uint32_t nP,
                                                             uint32_t T, uint64_t mask_lo, uint64_t mask_hi,
                                                             impop_haplotype_stats *__restrict__ rec, uint32_t *__restrict__ repsz,
                                                             uint32_t *__restrict__ class_of, uint32_t *__restrict__ sizes,
                                                             uint32_t *__restrict__ err) {
    extern __shared__ unsigned long long hap_lds[];
    unsigned long long *key = hap_lds;
    uint32_t *slot = reinterpret_cast<uint32_t *>(key + 2 * (size_t)nP);
    uint32_t *tab = slot + nP, *smin = tab + T;
    const uint32_t tid = threadIdx.x;
    const HapWin w = wins[blockIdx.x];
    for (uint32_t s = tid; s < T; s += HAP_T) {
        tab[s] = HAP_NONE;
        smin[s] = HAP_NONE;
    }
    for (uint32_t i = tid; i < nP; i += HAP_T) {
        uint64_t lo = 0, hi = 0;
        for (uint32_t t = w.t0; t < w.t1; ++t) {
            const uint64_t *src = fp + ((uint64_t)t * nP + i) * 2;
            lo ^= src[0];
            hi ^= src[1];
        }
        key[2 * i] = lo & mask_lo;
        key[2 * i + 1] = hi & mask_hi;
    }
    __syncthreads();
    // the first member to claim a slot owns it; members of equal key meet there (T > classes: a free slot always exists)
    for (uint32_t i = tid; i < nP; i += HAP_T) {
        const uint64_t lo = key[2 * i], hi = key[2 * i + 1];
        uint32_t h = (uint32_t)mix64(lo ^ (hi * 0x9E3779B97F4A7C15ull)) & (T - 1);
        for (;;) {
            const uint32_t old = atomicCAS(&tab[h], HAP_NONE, i);
            const uint32_t owner = old == HAP_NONE ? i : old;
            if (key[2 * owner] == lo && key[2 * owner + 1] == hi) break;
            h = (h + 1) & (T - 1);
        }
        slot[i] = h;
        atomicMin(&smin[h], i);
    }
    __syncthreads();
    for (uint32_t i = tid; i < nP; i += HAP_T) slot[i] = smin[slot[i]];  // now rep(i)
    uint32_t *scratch = reinterpret_cast<uint32_t *>(key);
    const uint64_t o = (uint64_t)blockIdx.x * nP;
    hap_emit(slot, scratch, scratch + nP, scratch + 2 * (size_t)nP, nP, w.n_sites, rec + blockIdx.x, repsz + o, class_of ? class_of + o : nullptr,
             sizes ? sizes + o : nullptr, err);
}

// grid = (window, tile) items of the chunk.  Dynamic LDS: repsz 4 nP | one row of 64-site words per wave, 8 nP each.
__global__ __launch_bounds__(HAP_T) void hap_verify_kernel(const uint32_t *__restrict__ sb, const uint64_t *__restrict__ rare,
                                                           const ScanTile *__restrict__ tiles, const HapItem *__restrict__ items,
                                                           uint32_t wps, uint32_t G, uint32_t r, const int32_t *__restrict__ ppos,
                                                           const uint32_t *__restrict__ pmask, uint32_t n_pad, uint32_t nP,
                                                           const impop_haplotype_stats *__restrict__ rec, const uint32_t *__restrict__ repsz,
                                                           uint32_t *__restrict__ flags) {
    extern __shared__ unsigned long long hap_lds[];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = (uint32_t)__builtin_amdgcn_readfirstlane(tid >> 6);
    const HapItem it = items[blockIdx.x];
    if (rec[it.win].n_distinct == nP) return;  // every member is its own representative: nothing to compare
    unsigned long long *words = hap_lds + (size_t)wave * nP;
    uint32_t *rs = reinterpret_cast<uint32_t *>(hap_lds + 4 * (size_t)nP);
    for (uint32_t i = tid; i < nP; i += HAP_T) rs[i] = repsz[(uint64_t)it.win * nP + i];
    __syncthreads();
    const ScanTile t = tiles[it.tile];
    const TileBlocks tb = tile_blocks_of(t);
    const uint64_t b0 = tb.b0, b1 = tb.b1;
    bool bad = false;
    for (uint64_t bb = b0; bb < b1; bb += 4) {  // the same trip count for every wave: the barriers are workgroup-wide
        const uint64_t b = bb + wave;
        if (b < b1)
            hap_block_words(sb + b * 64ull * wps, G, r, lane, hap_edge(t, b), ppos, pmask,
                            [&](uint32_t pp, uint64_t word) { words[pp] = word; });
        __syncthreads();
        if (b < b1)
            for (uint32_t i = lane; i < nP; i += 64) {
                const uint32_t rp = rs[i] & 0xFFFFu;
                bad |= words[i] != words[rp];
            }
        __syncthreads();
    }
    // rare entries: a class is listed as a whole or not at all — every listed member's representative is listed, and a listed
    // representative finds its whole class among the listed
    for (uint64_t e = t.rare_begin + tid; e < t.rare_end; e += HAP_T) {
        int32_t pp[IMPOP_RARE_MAX];
        hap_rare_members(stream_load(rare + e), ppos, n_pad, pp);
        int32_t rp[IMPOP_RARE_MAX];
#pragma unroll
        for (uint32_t i = 0; i < IMPOP_RARE_MAX; ++i) rp[i] = pp[i] >= 0 ? (int32_t)(rs[pp[i]] & 0xFFFFu) : -1;
#pragma unroll
        for (uint32_t i = 0; i < IMPOP_RARE_MAX; ++i)
            if (pp[i] >= 0) {
                uint32_t same = 0;
                bool rep_listed = false;
#pragma unroll
                for (uint32_t j = 0; j < IMPOP_RARE_MAX; ++j) {
                    rep_listed |= pp[j] == rp[i];
                    same += rp[j] == rp[i];
                }
                bad |= !rep_listed || same != (rs[pp[i]] >> 16);
            }
    }
    if (bad) flags[it.win] = 1u;
}

// grid = windows of the chunk; only flagged ones work.  Dynamic LDS: rep | eq | cnt | rank_of (4 nP each) | sortbuf.
__global__ __launch_bounds__(HAP_T) void hap_exact_kernel(const uint32_t *__restrict__ sb, const uint64_t *__restrict__ rare,
                                                          const ScanTile *__restrict__ tiles, const HapWin *__restrict__ wins, uint32_t wps,
                                                          uint32_t G, uint32_t r, const int32_t *__restrict__ ppos,
                                                          const uint32_t *__restrict__ pmask, const uint32_t *__restrict__ idx, uint32_t n_pad,
                                                          uint32_t nP, const uint32_t *__restrict__ flags,
                                                          impop_haplotype_stats *__restrict__ rec, uint32_t *__restrict__ repsz,
                                                          uint32_t *__restrict__ class_of, uint32_t *__restrict__ sizes,
                                                          uint32_t *__restrict__ err) {
    extern __shared__ unsigned long long hap_lds[];
    __shared__ uint32_t s_min;
    if (flags[blockIdx.x] == 0u) return;
    uint32_t *rep = reinterpret_cast<uint32_t *>(hap_lds), *eq = rep + nP;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = (uint32_t)__builtin_amdgcn_readfirstlane(tid >> 6);
    const HapWin w = wins[blockIdx.x];
    for (uint32_t i = tid; i < nP; i += HAP_T) rep[i] = HAP_NONE;
    for (uint32_t pass = 0; pass < nP; ++pass) {
        if (tid == 0) s_min = HAP_NONE;
        __syncthreads();
        uint32_t mine = HAP_NONE;
        for (uint32_t i = tid; i < nP; i += HAP_T)
            if (rep[i] == HAP_NONE) {
                mine = i;
                break;
            }
        if (mine != HAP_NONE) atomicMin(&s_min, mine);
        __syncthreads();
        const uint32_t cur = s_min;  // the smallest unassigned member represents the next class
        if (cur == HAP_NONE) break;
        for (uint32_t i = tid; i < nP; i += HAP_T) eq[i] = rep[i] == HAP_NONE;
        __syncthreads();
        const uint32_t ch = idx[cur];  // its row of the matrix
        for (uint32_t tt = w.t0; tt < w.t1; ++tt) {
            const ScanTile t = tiles[tt];
            const TileBlocks tb = tile_blocks_of(t);
            const uint64_t b0 = tb.b0, b1 = tb.b1;
            for (uint64_t b = b0 + wave; b < b1; b += 4) {
                const uint64_t edge = hap_edge(t, b);
                const uint32_t d = sb[sb_index(wps, G, r, b, lane, ch >> 5)];
                const uint64_t mine_w = __ballot((d >> (ch & 31u)) & 1u) & edge;
                hap_block_words(sb + b * 64ull * wps, G, r, lane, edge, ppos, pmask, [&](uint32_t pp, uint64_t word) {
                    if (word != mine_w) eq[pp] = 0u;
                });
            }
            for (uint64_t e = t.rare_begin + tid; e < t.rare_end; e += HAP_T) {
                const uint64_t v = stream_load(rare + e);
                int32_t pp[IMPOP_RARE_MAX];
                hap_rare_members(v, ppos, n_pad, pp);
                const bool listed = pp[0] == (int32_t)cur || pp[1] == (int32_t)cur || pp[2] == (int32_t)cur;
                if (!listed) {
#pragma unroll
                    for (uint32_t i = 0; i < IMPOP_RARE_MAX; ++i)
                        if (pp[i] >= 0) eq[pp[i]] = 0u;
                } else {
                    for (uint32_t i = 0; i < nP; ++i)
                        if ((int32_t)i != pp[0] && (int32_t)i != pp[1] && (int32_t)i != pp[2]) eq[i] = 0u;
                }
            }
        }
        __syncthreads();
        for (uint32_t i = tid; i < nP; i += HAP_T)
            if (eq[i] || i == cur) rep[i] = cur;
        __syncthreads();
    }
    __syncthreads();
    bool left = false;
    for (uint32_t i = tid; i < nP; i += HAP_T)
        if (rep[i] == HAP_NONE) {
            left = true;
            rep[i] = i;
        }
    if (left) atomicOr(err, DEV_ERR_HAPSCAN);
    const uint64_t o = (uint64_t)blockIdx.x * nP;
    hap_emit(rep, eq + nP, eq + 2 * (size_t)nP, eq + 3 * (size_t)nP, nP, w.n_sites, rec + blockIdx.x, repsz + o, class_of ? class_of + o : nullptr,
             sizes ? sizes + o : nullptr, err);
}

static uint32_t pow2_at_least(uint32_t x) {
    uint32_t p = 1;
    while (p < x) p <<= 1;
    return p;
}

// IMPOP_HAPSCAN_KEY_BITS=n (1..128, default 128): fingerprints truncated to n bits, so that tests reach the verify and exact paths
static uint32_t hapscan_key_bits() {
    const char *e = getenv("IMPOP_HAPSCAN_KEY_BITS");
    if (!e || !*e) return 128;
    const long v = strtol(e, nullptr, 10);
    return v < 1 ? 1u : v > 128 ? 128u : (uint32_t)v;
}

}  // namespace impop

using namespace impop;

IMPOP_API int impop_haplotype_scan(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows,
                                   const uint64_t *mask_p, const impop_haplotype_params *params, impop_haplotype_stats *out_host,
                                   uint32_t *class_of, uint32_t *sizes) {
    static_assert(sizeof(impop_haplotype_stats) == 64 && sizeof(impop_haplotype_params) == 16, "ABI layout");
    REQUIRE(ctx && m && params, "impop_haplotype_scan: NULL argument");
    REQUIRE(params->struct_size == sizeof(impop_haplotype_params), "impop_haplotype_params.struct_size mismatch");
    REQUIRE(m->device == ctx->device, "impop_haplotype_scan: matrix lives on device %d, context on %d", m->device, ctx->device);
    const uint32_t wps = m->g.wps, n_pad = wps * 32;
    const MemberSet P = member_set(mask_p, m->g.n_hap, wps);
    const uint32_t nP = P.size();
    REQUIRE(nP > 0, "impop_haplotype_scan: the mask selects no haplotype");
    if (nP > IMPOP_HAPLOTYPE_MAX_N) {
        set_error("impop_haplotype_scan: %u members exceed the LDS-resident grouping limit (%u)", nP, (uint32_t)IMPOP_HAPLOTYPE_MAX_N);
        return IMPOP_E_UNSUPPORTED;
    }
    if (!n_windows) return IMPOP_OK;
    REQUIRE(windows && out_host, "impop_haplotype_scan: NULL windows/out");
    int rc = check_windows("impop_haplotype_scan", m, windows, n_windows);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    ScanRoute rt;
    rc = scan_route("impop_haplotype_scan", ctx, m, windows, n_windows, 0, rt);
    if (rc) return rc;

    // device bytes of a chunk: 16 nP per tile of fingerprints, 12 nP per window of tables, 8 per item of the verify kernel
    const TileCosts costs{16ull * nP, 12ull * nP + sizeof(impop_haplotype_stats) + sizeof(HapWin) + 4, sizeof(HapItem)};
    const std::vector<TiledChunk> chunks =
        plan_tiled_chunks(rt.wins.data(), n_windows, rt.tiles.size(), chunk_budget(params->max_chunk_bytes), 0, costs);
    const size_t max_tiles = max_over(chunks, [](const TiledChunk &c) { return c.tiles.size(); }),
                 max_wins = max_over(chunks, [](const TiledChunk &c) { return c.w_end - c.w_begin; }),
                 max_items = max_over(chunks, [](const TiledChunk &c) { return c.items; });
    REQUIRE(max_tiles < 0x7FFFFFFFull && max_items < 0x7FFFFFFFull && max_wins < 0x7FFFFFFFull,
            "impop_haplotype_scan: a chunk of %zu tiles / %zu window tiles exceeds one launch", max_tiles, max_items);
    REQUIRE((uint64_t)max_tiles * 16ull * nP <= (64ull << 30), "impop_haplotype_scan: a window needs %llu MiB of tile fingerprints",
            (unsigned long long)(((uint64_t)max_tiles * 16ull * nP) >> 20));

    // device: idx | ppos | pmask | tiles | windows | items (up, through the page-locked staging with the same offsets) |
    // records | flags (down, staged) | fingerprints | rep-and-size, class_of, sizes tables
    Carve L;
    const size_t o_idx = L.take<uint32_t>(nP), o_ppos = L.take<int32_t>(n_pad), o_pmask = L.take<uint32_t>(wps), o_fixed = L.total(),
                 o_tiles = L.take<ScanTile>(max_tiles), o_wins = L.take<HapWin>(max_wins), o_items = L.take<HapItem>(max_items),
                 o_rec = L.take<impop_haplotype_stats>(max_wins), o_flags = L.take<uint32_t>(max_wins), staged = L.total(),
                 o_fp = L.take<uint64_t>(max_tiles * 2 * nP), o_repsz = L.take<uint32_t>(max_wins * nP),
                 o_cls = L.take<uint32_t>(class_of ? max_wins * nP : 0), o_sz = L.take<uint32_t>(sizes ? max_wins * nP : 0);
    void *d = nullptr, *pin = nullptr;
    rc = ctx_scratch(ctx, L.total(), &d);
    if (rc) return rc;
    rc = ctx_pinned(ctx, staged, &pin);
    if (rc) return rc;
    const ChunkRun run{ctx, "impop_haplotype_scan", (char *)d, (char *)pin};
    char *dc = run.dc, *hc = run.hc;
    memcpy(hc + o_idx, P.idx.data(), (size_t)nP * 4);
    memcpy(hc + o_ppos, P.ppos.data(), (size_t)n_pad * 4);
    memcpy(hc + o_pmask, P.bits.data(), (size_t)wps * 4);
    if ((rc = run.up(0, o_fixed))) return rc;

    const uint32_t T = std::max<uint32_t>(64, pow2_at_least(2 * nP));
    const size_t lds_fp = (size_t)nP * 16, lds_cls = (size_t)nP * 20 + (size_t)T * 8, lds_ver = (size_t)nP * 36,
                 lds_exact = (size_t)nP * 16 + (size_t)pow2_at_least(nP) * 4;
    if ((rc = lds_opt_in(hap_fingerprint_kernel, lds_fp)) || (rc = lds_opt_in(hap_classify_kernel, lds_cls)) ||
        (rc = lds_opt_in(hap_verify_kernel, lds_ver)) || (rc = lds_opt_in(hap_exact_kernel, lds_exact)))
        return rc;
    const uint32_t bits = hapscan_key_bits();
    const uint64_t mask_lo = bits >= 64 ? ~0ull : (1ull << bits) - 1ull;
    const uint64_t mask_hi = bits <= 64 ? 0ull : bits >= 128 ? ~0ull : (1ull << (bits - 64)) - 1ull;

    const int32_t *d_ppos = (const int32_t *)(dc + o_ppos);
    const uint32_t *d_pmask = (const uint32_t *)(dc + o_pmask), *d_idx = (const uint32_t *)(dc + o_idx);
    const ScanTile *d_tiles = (const ScanTile *)(dc + o_tiles);
    const HapWin *d_wins = (const HapWin *)(dc + o_wins);
    impop_haplotype_stats *d_rec = (impop_haplotype_stats *)(dc + o_rec);
    uint32_t *d_flags = (uint32_t *)(dc + o_flags), *d_repsz = (uint32_t *)(dc + o_repsz);
    uint32_t *d_cls = class_of ? (uint32_t *)(dc + o_cls) : nullptr, *d_sz = sizes ? (uint32_t *)(dc + o_sz) : nullptr;
    ScanTile *h_tiles = (ScanTile *)(hc + o_tiles);
    HapWin *h_wins = (HapWin *)(hc + o_wins);
    HapItem *h_items = (HapItem *)(hc + o_items);
    EventPairs *timer = ctx->timers + impop_ctx::T_HAP;
    uint64_t launches = 0, collided = 0, bytes_streamed = 0, tiles_run = 0;
    for (const TiledChunk &c : chunks) {
        const size_t nt = c.tiles.size(), cnt = c.w_end - c.w_begin, ni = c.items;
        for (size_t k = 0; k < nt; ++k) {
            h_tiles[k] = rt.tiles[c.tiles[k]];
            bytes_streamed += tile_bytes_streamed(h_tiles[k], wps);
        }
        for (size_t k = 0, item = 0; k < cnt; ++k) {
            const WinDesc &w = rt.wins[c.w_begin + k];
            const uint32_t l0 = c.l0[k], tiles_k = (uint32_t)(w.t1 - w.t0);
            h_wins[k] = HapWin{l0, l0 + tiles_k, (uint32_t)w.n_sites, 0u};
            for (uint32_t t = 0; t < tiles_k; ++t) h_items[item++] = HapItem{(uint32_t)k, l0 + t};
        }
        if ((rc = run.up(o_tiles, o_rec))) return rc;  // from the tiles to the end of the items
        HIP_TRY(hipMemsetAsync(d_flags, 0, cnt * 4, ctx->stream));
        if (nt) {
            if ((rc = run.timed(timer[0], [&] {
                hipLaunchKernelGGL(hap_fingerprint_kernel, dim3((uint32_t)nt), dim3(HAP_T), lds_fp, ctx->stream, rt.sb, rt.rare, d_tiles, wps,
                                   m->g.G, m->g.r, d_ppos, d_pmask, n_pad, nP, (uint64_t *)(dc + o_fp));
            }))) return rc;
            ++launches;
        }
        if ((rc = run.timed(timer[1], [&] {
            hipLaunchKernelGGL(hap_classify_kernel, dim3((uint32_t)cnt), dim3(HAP_T), lds_cls, ctx->stream, (const uint64_t *)(dc + o_fp),
                               d_wins, nP, T, mask_lo, mask_hi, d_rec, d_repsz, d_cls, d_sz, ctx->d_err);
        }))) return rc;
        ++launches;
        if (ni) {
            if ((rc = run.timed(timer[2], [&] {
                hipLaunchKernelGGL(hap_verify_kernel, dim3((uint32_t)ni), dim3(HAP_T), lds_ver, ctx->stream, rt.sb, rt.rare, d_tiles,
                                   (const HapItem *)(dc + o_items), wps, m->g.G, m->g.r, d_ppos, d_pmask, n_pad, nP, d_rec, d_repsz, d_flags);
                hipLaunchKernelGGL(hap_exact_kernel, dim3((uint32_t)cnt), dim3(HAP_T), lds_exact, ctx->stream, rt.sb, rt.rare, d_tiles, d_wins,
                                   wps, m->g.G, m->g.r, d_ppos, d_pmask, d_idx, n_pad, nP, d_flags, d_rec, d_repsz, d_cls, d_sz, ctx->d_err);
            }))) return rc;
            launches += 2;
        }
        if (class_of) HIP_TRY(hipMemcpyAsync(class_of + c.w_begin * nP, d_cls, cnt * nP * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (sizes) HIP_TRY(hipMemcpyAsync(sizes + c.w_begin * nP, d_sz, cnt * nP * 4, hipMemcpyDeviceToHost, ctx->stream));
        if ((rc = run.finish(o_rec, staged))) return rc;  // records and flags
        const impop_haplotype_stats *rv = (const impop_haplotype_stats *)(hc + o_rec);
        const uint32_t *fv = (const uint32_t *)(hc + o_flags);
        for (size_t k = 0; k < cnt; ++k) {
            impop_haplotype_stats o = rv[k];
            const double nn = (double)o.n_members;
            o.h1 = (double)o.sum_sq / (nn * nn);
            o.h12 = o.h1 + 2.0 * ((double)o.largest / nn) * ((double)o.second / nn);
            o.h2_h1 = (o.h1 - ((double)o.largest / nn) * ((double)o.largest / nn)) / o.h1;
            o.hap_diversity = o.n_members < 2 ? 0.0 : (1.0 - o.h1) * nn / (nn - 1.0);
            out_host[c.w_begin + k] = o;
            collided += fv[k] != 0;
        }
        tiles_run += nt;
    }
    if (trace_on()) {
        fprintf(stderr, "[impop_haplotype_scan] route=%s windows=%llu tiles=%llu chunks=%llu launches=%llu collided_windows=%llu bytes_streamed=%llu\n",
                rt.indexed ? (rt.split ? "indexed+rare" : "indexed") : m->compact ? "compact" : "dense", (unsigned long long)n_windows,
                (unsigned long long)tiles_run, (unsigned long long)chunks.size(), (unsigned long long)launches, (unsigned long long)collided,
                (unsigned long long)bytes_streamed);
        fflush(stderr);
    }
    return IMPOP_OK;
}

IMPOP_API int impop_ctx_haplotype_elapsed(impop_ctx *ctx, double kernel_ms[3], uint64_t *chunks) {
    REQUIRE(ctx && kernel_ms, "impop_ctx_haplotype_elapsed: NULL argument");
    return ctx_timers_elapsed(ctx, impop_ctx::T_HAP, 3, 1, kernel_ms, chunks);
}
