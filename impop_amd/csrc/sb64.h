// sb64.h — device-side reading of one 64-site block of the SB64 layout (internal.h): a lane's full 16-byte granules and
// the last granule's r = 1..3 dwords.  Every helper is forced inline and keeps the caller's wave-uniform predicates
// (g, nb, G, r) wave-uniform, so a kernel's loads go out in the order its source lists them: all of a batch, then the use.
#pragma once
#include "internal.h"

namespace impop {

// Measured (tools/tune_scan.py, 465 x 75 M sites, interleaved rounds): nt loads 6.65-6.68 TB/s algorithmic vs
// 5.9-6.07 TB/s with default-policy loads (+10 %).
#ifndef IMPOP_SCAN_NT
#define IMPOP_SCAN_NT 1        // 1: non-temporal (streaming) loads for the once-read matrix
#endif

typedef uint32_t u32v4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32v2 __attribute__((ext_vector_type(2)));

template <typename T>
__device__ __forceinline__ T stream_load(const T *p) {
#if IMPOP_SCAN_NT
    return __builtin_nontemporal_load(p);
#else
    return *p;
#endif
}
// STREAM: the scan kernels' once-read stream; else a plain load (the layout kernels)
template <bool STREAM, typename T>
__device__ __forceinline__ T sb_load(const T *p) {
    if constexpr (STREAM) return stream_load(p);
    else return *p;
}

// full 16-byte granules of a site: all G when the last one holds 4 dwords (r == 4: its addressing is the full granules'),
// else all but the last, whose r = 1..3 dwords per site are read one by one
__device__ __forceinline__ uint32_t sb_full_granules(uint32_t G, uint32_t r) { return r == 4 ? G : G - 1; }

// site l's full granule g of the block at blk: the wave's 64 of them are one coalesced 1 KiB access
__device__ __forceinline__ const u32v4 *sb_granule(const uint32_t *blk, uint32_t g, uint32_t l) {
    return reinterpret_cast<const u32v4 *>(blk + (uint64_t)g * 256 + l * 4);
}
__device__ __forceinline__ u32v4 *sb_granule(uint32_t *blk, uint32_t g, uint32_t l) {
    return reinterpret_cast<u32v4 *>(blk + (uint64_t)g * 256 + l * 4);
}
// site l's dwords of the last, shorter granule (meaningful when sb_full_granules < G)
__device__ __forceinline__ const uint32_t *sb_tail(const uint32_t *blk, uint32_t G, uint32_t r, uint32_t l) {
    return blk + (uint64_t)sb_full_granules(G, r) * 256 + l * r;
}
__device__ __forceinline__ uint32_t *sb_tail(uint32_t *blk, uint32_t G, uint32_t r, uint32_t l) {
    return blk + (uint64_t)sb_full_granules(G, r) * 256 + l * r;
}

// the last granule's r = 1..3 dwords of site l -> tl[0..r) (nothing when r == 4).  Issue it BEFORE the batches are consumed:
// read behind them the tail costs one more memory latency per block.
template <bool STREAM = true>
__device__ __forceinline__ void sb_load_tail(const uint32_t *blk, uint32_t G, uint32_t r, uint32_t l, uint32_t (&tl)[3]) {
    const uint32_t *last = sb_tail(blk, G, r, l);
#pragma unroll
    for (int j = 0; j < 3; ++j)
        if (r < 4 && (uint32_t)j < r) tl[j] = sb_load<STREAM>(last + j);
}
// k = dword index of tl[j] in the site; f(k, dword) for the dwords sb_load_tail read
template <typename F>
__device__ __forceinline__ void sb_use_tail(uint32_t G, uint32_t r, const uint32_t (&tl)[3], F f) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
        if (r < 4 && (uint32_t)j < r) f(4 * (G - 1) + j, tl[j]);
}

// full granules g .. g + nb (nb <= U, wave-uniform) of site l -> v[0..nb): all loads out before the first is consumed
template <int U, bool STREAM = true>
__device__ __forceinline__ void sb_load_granules(const uint32_t *blk, uint32_t g, uint32_t nb, uint32_t l, u32v4 (&v)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u)
        if ((uint32_t)u < nb) v[u] = sb_load<STREAM>(sb_granule(blk, g + u, l));
}

// f(k, dword k) for every dword of site l: the tail and then four granules at a time in flight (a site of <= 512
// haplotypes is one batch: every load of the block is out before the first is consumed)
template <bool STREAM, typename F>
__device__ __forceinline__ void sb_for_each_dword(const uint32_t *blk, uint32_t G, uint32_t r, uint32_t l, F f) {
    const uint32_t Gf = sb_full_granules(G, r);
    uint32_t tl[3] = {0u, 0u, 0u};
    sb_load_tail<STREAM>(blk, G, r, l, tl);
    for (uint32_t g = 0; g < Gf; g += 4) {
        const uint32_t nb = Gf - g < 4u ? Gf - g : 4u;
        u32v4 v[4];
        sb_load_granules<4, STREAM>(blk, g, nb, l, v);
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if ((uint32_t)u < nb) {
                const uint32_t k = 4 * (g + u);
                f(k, v[u].x); f(k + 1, v[u].y); f(k + 2, v[u].z); f(k + 3, v[u].w);
            }
    }
    sb_use_tail(G, r, tl, f);
}

// compile-time shape (the fixed-WPS scan kernel): all WPS dwords of row i of a block of `rows` rows at blk, interleaved by
// granule as an SB64 block is (rows = 64) — granule g of row i at dword (g rows + i) 4, the last granule's R dwords at
// (G - 1) rows 4 + i R.  rows a multiple of 4 keeps every granule section 64-byte aligned to blk (the tile digest, tile_digest.h)
template <int WPS, bool STREAM>
__device__ __forceinline__ void load_row(const uint32_t *__restrict__ blk, uint32_t rows, uint32_t i, uint32_t (&w)[WPS]) {
    constexpr int G = (WPS + 3) / 4;
    constexpr int R = WPS - 4 * (G - 1);
#pragma unroll
    for (int g = 0; g < G - 1; ++g) {
        const u32v4 v = sb_load<STREAM>(reinterpret_cast<const u32v4 *>(blk + (uint64_t)g * (rows * 4) + i * 4));
        w[4 * g + 0] = v.x; w[4 * g + 1] = v.y; w[4 * g + 2] = v.z; w[4 * g + 3] = v.w;
    }
    const uint32_t *last = blk + (G - 1) * (rows * 4) + i * R;
    if constexpr (R == 4) {
        const u32v4 v = sb_load<STREAM>(reinterpret_cast<const u32v4 *>(last));
        w[4 * (G - 1) + 0] = v.x; w[4 * (G - 1) + 1] = v.y; w[4 * (G - 1) + 2] = v.z; w[4 * (G - 1) + 3] = v.w;
    } else if constexpr (R == 3) {
        // 12-byte, 4-byte-aligned: three dwords (the backend merges them into one dwordx3)
        w[4 * (G - 1) + 0] = sb_load<STREAM>(last);
        w[4 * (G - 1) + 1] = sb_load<STREAM>(last + 1);
        w[4 * (G - 1) + 2] = sb_load<STREAM>(last + 2);
    } else if constexpr (R == 2) {
        const u32v2 v = sb_load<STREAM>(reinterpret_cast<const u32v2 *>(last));
        w[4 * (G - 1) + 0] = v.x; w[4 * (G - 1) + 1] = v.y;
    } else {
        w[4 * (G - 1)] = sb_load<STREAM>(last);
    }
}
// all WPS dwords of site `lane` of an SB64 block
template <int WPS>
__device__ __forceinline__ void load_site(const uint32_t *__restrict__ blk, uint32_t lane, uint32_t (&w)[WPS]) {
    load_row<WPS, true>(blk, 64u, lane, w);
}

}  // namespace impop
