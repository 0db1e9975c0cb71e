// hap_words.h — what the streaming kernels over scan_route's tiles share (scan.hip, hapscan.hip, diploid.hip, and through
// pop_stream.h dstat.hip): a tile's 64-site blocks (tile_blocks_of, the one block-range helper) with its edges masked, the ballot
// transpose of a block into per-haplotype 64-site words, the members a rare entry lists and how many of them a population mask holds.
#pragma once
#include "device_utils.h"
#include "internal.h"
#include "sb64.h"
#include "scan_route.h"

namespace impop {

// the blocks [b0, b1) a tile's sites lie in, and this thread's lane and wave; the wave index goes through readfirstlane so that
// block addresses and loops formed from it stay scalar (SGPR) state.  The 256-thread kernels of scan.hip and pop_stream.h give
// wave w the blocks b0 + w, b0 + w + 4, ...; hapscan.hip and diploid.hip split a tile their own way and take b0, b1 alone.
struct TileBlocks {
    uint64_t b0, b1;
    uint32_t lane, wave;
};
__device__ __forceinline__ TileBlocks tile_blocks_of(const ScanTile &t) {
    const uint64_t b0 = t.site_begin >> 6;
    return {b0, t.site_end > t.site_begin ? (t.site_end + 63) >> 6 : b0, threadIdx.x & 63,
            (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)};
}
// the sites of block b inside the tile
__device__ __forceinline__ uint64_t hap_edge(const ScanTile &t, uint64_t b) {
    uint64_t edge = ~0ull;
    if (b * 64 < t.site_begin) edge &= ~0ull << (t.site_begin - b * 64);
    if (t.site_end - b * 64 < 64) edge &= (1ull << (t.site_end - b * 64)) - 1ull;
    return edge;
}

// f(pp, word) for every member of P (pp = its position in P) with its 64-site word of block blk, sites outside `edge` cleared.
// Dword columns without a member are skipped (pmask[k], wave-uniform).  Called by whole waves; lanes 0..31 run f.
template <typename F>
__device__ __forceinline__ void hap_block_words(const uint32_t *blk, uint32_t G, uint32_t r, uint32_t lane, uint64_t edge,
                                                const int32_t *__restrict__ ppos, const uint32_t *__restrict__ pmask, F f) {
    sb_for_each_dword<true>(blk, G, r, lane, [&](uint32_t k, uint32_t w) {
        if (__builtin_amdgcn_readfirstlane(pmask[k]) == 0u) return;
        const uint64_t word = ballot_transpose32(w, lane) & edge;
        if (lane < 32) {
            const int32_t pp = ppos[32 * k + lane];
            if (pp >= 0) f((uint32_t)pp, word);
        }
    });
}

// A rare entry (internal.h, rare_pack) lists the m <= 3 carriers of its minor allele: how many of them belong to a population
// comes from bit tests on its mask in LDS (per-lane addresses, a few dwords)
__device__ __forceinline__ uint32_t rare_listed_in(const uint32_t *mask_lds, uint64_t e) {
    const uint32_t m = rare_count(e);
    uint32_t in = 0;
#pragma unroll
    for (uint32_t i = 0; i < IMPOP_RARE_MAX; ++i)
        if (i < m) {
            const uint32_t h = rare_slot(e, i);
            in += (mask_lds[h >> 5] >> (h & 31u)) & 1u;
        }
    return in;
}

// P positions of the haplotypes a rare entry lists (-1: not in P, or an unused slot)
__device__ __forceinline__ void hap_rare_members(uint64_t v, const int32_t *__restrict__ ppos, uint32_t n_pad, int32_t (&pp)[IMPOP_RARE_MAX]) {
    const uint32_t m = rare_count(v);
#pragma unroll
    for (uint32_t i = 0; i < IMPOP_RARE_MAX; ++i) {
        const uint32_t h = rare_slot(v, i);
        pp[i] = (i < m && h < n_pad) ? ppos[h] : -1;
    }
}

}  // namespace impop
