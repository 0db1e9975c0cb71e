// ibs_transpose.h — the word-major transposed stream shared by impop_ibs_scan / impop_ibd_scan (ibs.hip) and impop_paint_scan
// (paint.hip): [64-site block of a chunk][row] uint64, rows = the haplotypes of a member set (win_chunks.h: ppos, bits), made per
// chunk of blocks from the site-major SB64 rows.  The range's edges are masked off here, so a reader sees no difference outside it.
#pragma once
#include "device_utils.h"
#include "internal.h"

namespace impop {

// grid = ceil(len / 4): wave = one 64-site block of the chunk.  ppos[h] = row of haplotype h or -1 (padding rows included),
// pmask[k] = the rows of dword column k.  [cb, ce) = the range's columns: everything outside is written as 0.
static __global__ __launch_bounds__(256) void ibs_transpose_kernel(const uint32_t *__restrict__ sb, uint32_t wps, uint32_t G, uint32_t r,
                                                                   const int32_t *__restrict__ ppos, const uint32_t *__restrict__ pmask,
                                                                   uint64_t blk_abs0, uint64_t len, uint64_t cb, uint64_t ce, uint32_t stride,
                                                                   uint64_t *__restrict__ wm) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t bi = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (bi >= len) return;  // wave-uniform
    const uint64_t B = blk_abs0 + bi;
    uint64_t edge = ~0ull;
    if (B * 64 < cb) edge &= ~0ull << (cb - B * 64);
    if (ce - B * 64 < 64) edge &= (1ull << (ce - B * 64)) - 1ull;
    for (uint32_t k = 0; k < wps; ++k) {
        const uint32_t pm = (uint32_t)__builtin_amdgcn_readfirstlane(pmask[k]);
        if (pm == 0u) continue;
        const uint64_t keep = ballot_transpose32(sb[sb_index(wps, G, r, B, lane, k)], lane) & edge;
        if (lane < 32) {
            const int32_t pp = ppos[32 * k + lane];
            if (pp >= 0) wm[bi * stride + (uint32_t)pp] = keep;
        }
    }
}

}  // namespace impop
