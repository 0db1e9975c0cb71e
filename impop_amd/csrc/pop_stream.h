// pop_stream.h — the streaming pass of the K-population kernels (scan_multi_kernel in scan.hip, dstat_tiles_kernel in dstat.hip),
// once: the masks of all K populations in LDS (K x wps4 dwords, read back as broadcast ds_read_b128), a lane per site, four
// granules in flight per wave, the rare entries of a split index, and the four-wave reduction that writes a tile's row of 64-bit
// partials.  What a site's K counts add is the kernel's own: it arrives as a lambda and keeps its accumulators in the kernel.
// Forced-inline templates like sb64.h / hap_words.h; 256-thread workgroups.
#pragma once
#include "device_utils.h"
#include "hap_words.h"
#include "sb64.h"

namespace impop {

// masks (K x wps dwords) -> mk_lds (K x wps4, each mask padded with zeros to whole granules).  The caller keeps the __syncthreads().
template <int K>
__device__ __forceinline__ void pop_masks_to_lds(uint32_t *mk_lds, const uint32_t *__restrict__ masks, uint32_t wps) {
    const uint32_t wps4 = (wps + 3) & ~3u;
    for (uint32_t i = threadIdx.x; i < K * wps4; i += 256) {
        const uint32_t k = i / wps4, j = i % wps4;
        mk_lds[i] = j < wps ? masks[(uint64_t)k * wps + j] : 0u;
    }
}

// One tile (tb = tile_blocks_of(t), the kernel's one copy): on_site(c, s) with the K counts of every site s inside the tile, then
// (RARE) on_rare(c) with those of every rare entry, mirrored through pop_n[k] - m_k when the entry lists the carriers of 0.  c is
// a register array: the callees index it with compile-time constants only (a select between two of its elements would put it in
// scratch, see dstat_pick).
template <int K, bool RARE, typename OnSite, typename OnRare>
__device__ __forceinline__ void pop_stream_tile(const uint32_t *__restrict__ sb, const uint64_t *__restrict__ rare, const ScanTile &t,
                                                const TileBlocks &tb, const uint32_t *mk_lds, const uint32_t *__restrict__ pop_n,
                                                uint32_t wps, uint32_t G, uint32_t r, OnSite on_site, OnRare on_rare) {
    constexpr int MU = 4;  // granules in flight per wave
    const uint32_t wps4 = (wps + 3) & ~3u;
    const uint32_t Gf = sb_full_granules(G, r);
    auto count_batch = [&](uint32_t g, uint32_t nb, const u32v4 (&v)[MU], uint32_t (&c)[K]) {
#pragma unroll
        for (int u = 0; u < MU; ++u)
            if ((uint32_t)u < nb) {
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const u32v4 m4 = *reinterpret_cast<const u32v4 *>(mk_lds + k * wps4 + 4 * (g + u));
                    c[k] += __popc(v[u].x & m4.x) + __popc(v[u].y & m4.y) + __popc(v[u].z & m4.z) + __popc(v[u].w & m4.w);
                }
            }
    };
    // the last granule's r = 1..3 dwords per site are loaded TOGETHER with the batch (sb_load_tail)
    auto count_tail = [&](const uint32_t (&tl)[3], uint32_t (&c)[K]) {
        sb_use_tail(G, r, tl, [&](uint32_t j, uint32_t v) {
#pragma unroll
            for (int k = 0; k < K; ++k) c[k] += __popc(v & mk_lds[k * wps4 + j]);  // j: the dword's index in the site
        });
    };
    auto tally = [&](uint64_t b, const uint32_t (&c)[K]) {
        const uint64_t s = b * 64 + tb.lane;
        if (s >= t.site_begin && s < t.site_end) on_site(c, s);  // only the first / last block of a tile is partial
    };
    uint64_t b = tb.b0 + tb.wave;
    if (Gf <= (uint32_t)MU) {
        // <= 512 haplotypes: a block is one batch; two blocks (up to 8 wave loads) in flight per wave
        for (; b + 4 < tb.b1; b += 8) {
            const uint32_t *blk0 = sb + b * 64ull * wps, *blk1 = sb + (b + 4) * 64ull * wps;
            u32v4 v0[MU], v1[MU];
            uint32_t t0[3], t1[3];
            sb_load_granules(blk0, 0, Gf, tb.lane, v0);
            sb_load_tail(blk0, G, r, tb.lane, t0);
            sb_load_granules(blk1, 0, Gf, tb.lane, v1);
            sb_load_tail(blk1, G, r, tb.lane, t1);
            uint32_t c0[K], c1[K];
#pragma unroll
            for (int k = 0; k < K; ++k) { c0[k] = 0; c1[k] = 0; }
            count_batch(0, Gf, v0, c0);
            count_tail(t0, c0);
            tally(b, c0);
            count_batch(0, Gf, v1, c1);
            count_tail(t1, c1);
            tally(b + 4, c1);
        }
    }
    for (; b < tb.b1; b += 4) {
        const uint32_t *blk = sb + b * 64ull * wps;
        uint32_t c[K];
#pragma unroll
        for (int k = 0; k < K; ++k) c[k] = 0;
        uint32_t tl[3];
        sb_load_tail(blk, G, r, tb.lane, tl);
        for (uint32_t g = 0; g < Gf; g += MU) {
            const uint32_t nb = Gf - g < (uint32_t)MU ? Gf - g : (uint32_t)MU;
            u32v4 v[MU];
            sb_load_granules(blk, g, nb, tb.lane, v);
            count_batch(g, nb, v, c);
        }
        count_tail(tl, c);
        tally(b, c);
    }
    // rare entries of the split index (unweighted matrices only): each population's count from bit tests of the listed
    // haplotypes, mirrored through n_k - m_k when they carry 0
    if constexpr (RARE) {
        // the sizes are read here, not before the rows: dstat_tiles_kernel needs them nowhere else, and K fewer scalar registers
        // are live in its loops above (scan_multi_kernel keeps a copy of its own for its sums)
        uint32_t nk[K];
#pragma unroll
        for (int k = 0; k < K; ++k) nk[k] = pop_n[k];
        for (uint64_t e = t.rare_begin + threadIdx.x; e < t.rare_end; e += 256) {
            const uint64_t v = stream_load(rare + e);
            uint32_t c[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const uint32_t mk = rare_listed_in(mk_lds + k * wps4, v);
                c[k] = rare_lists_zeros(v) ? nk[k] - mk : mk;
            }
            on_rare(c);
        }
    }
}

// c[i] for a wave-uniform i: a chain of K selects (a register array has no run-time index).  The chain starts from a constant,
// not from c[0]: a select between two elements of c is folded into a load through a selected ADDRESS, which keeps c in scratch.
template <int K>
__device__ __forceinline__ uint32_t dstat_pick(const uint32_t (&c)[K], uint32_t i) {
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) v = i == (uint32_t)k ? c[k] : v;
    return v;
}

// wave_val(i), i = 0 .. NV - 1: the wave's sum of the tile's value i (wave_sum_u64, or wave_sum_u32 for a 32-bit counter).  The four
// waves' sums are added and the tile's row is written: out[blockIdx.x * NV + i].  No atomics: the same bits on every run.
// The sums go SUMS at a time with one lane-0 store block behind them: one value at a time puts a branch and a wait behind every
// butterfly, which cost dstat_tiles_kernel 8 % of its launch; all NV at once keeps every sum alive and doubled the VGPRs of
// scan_multi_kernel<8, true>.
template <int NV, typename WaveVal>
__device__ __forceinline__ void tile_partials_store(const TileBlocks &tb, uint64_t *__restrict__ out, WaveVal wave_val) {
    constexpr int SUMS = 7;
    __shared__ uint64_t red[4][NV];
#pragma unroll
    for (int i0 = 0; i0 < NV; i0 += SUMS) {
        uint64_t v[SUMS];
#pragma unroll
        for (int i = i0; i < NV && i < i0 + SUMS; ++i) v[i - i0] = wave_val(i);
        if (tb.lane == 0) {
#pragma unroll
            for (int i = i0; i < NV && i < i0 + SUMS; ++i) red[tb.wave][i] = v[i - i0];
        }
    }
    __syncthreads();
    if (threadIdx.x < NV)
        out[(uint64_t)blockIdx.x * NV + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

}  // namespace impop
