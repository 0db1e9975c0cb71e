// ld_select.h — the site selection shared by impop_ld_scan (ldscan.hip) and impop_recomb_scan (recomb.hip): which sites of a
// window qualify (minor-allele count among the members of P), which of them are used (the thinning rule, in one place), and their
// rows ANDed with P, their carrier counts and their original coordinates gathered into a chunk's scratch.
//   ld_select_kernel  one wave per 64-site block of a window: c = carriers among P of the lane's site, the ballot of
//                     min(c, |P| - c) >= min_mac over the window's sites -> one 64-bit qualifying mask per block.
//   ld_gather_kernel  one workgroup per window: q = the masks' popcount, a prefix over the threads' runs of blocks ranks every
//                     qualifying site, the sites of rank floor(k q / m) are kept; their rows, c and coordinates go to [row_off + k].
// A window's slots in the scratch start at row_off and number cap >= m: the caller lays them out.
#pragma once
#include <algorithm>

#include "device_utils.h"
#include "internal.h"
#include "sb64.h"

namespace impop {

constexpr int LD_T = 256;  // threads of the workgroups here

struct LdWin {          // a window of a chunk
    uint64_t s0, s1;    // its sites in d_sb
    uint64_t blk_off;   // its first qualifying mask in the chunk's mask array
    uint64_t row_off;   // its first slot in the chunk's rows / counts / coordinates
    uint32_t n_sites;   // W
    uint32_t cap;       // its slots: max_sites, or fewer where the window cannot hold that many sites
};

// the 64-site blocks a window touches; the grid's second dimension for the chunk whose longest window touches `longest` blocks
inline uint64_t ld_blocks(uint64_t s0, uint64_t s1) { return s1 > s0 ? ((s1 + 63) >> 6) - (s0 >> 6) : 0; }
inline uint32_t ld_select_slices(uint64_t longest) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((longest + 63) / 64, 1), 1024); }

// grid = (windows of the chunk, slices of a window's blocks)
static __global__ __launch_bounds__(LD_T) void ld_select_kernel(const uint32_t *__restrict__ sb, const LdWin *__restrict__ wins, uint32_t wps,
                                                                uint32_t G, uint32_t r, const uint32_t *__restrict__ pbits, uint32_t nP,
                                                                uint32_t min_mac, uint64_t *__restrict__ qmask) {
    const uint32_t lane = threadIdx.x & 63, wave = (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const LdWin w = wins[blockIdx.x];
    if (w.s1 <= w.s0) return;
    const uint64_t b0 = w.s0 >> 6, b1 = (w.s1 + 63) >> 6;
    for (uint64_t b = b0 + (uint64_t)blockIdx.y * 4 + wave; b < b1; b += 4ull * gridDim.y) {
        uint32_t c = 0;
        sb_for_each_dword<true>(sb + b * 64ull * wps, G, r, lane, [&](uint32_t k, uint32_t d) { c += __popc(d & pbits[k]); });
        const uint64_t site = b * 64 + lane;
        const uint32_t mac = c < nP - c ? c : nP - c;
        const uint64_t mask = __ballot(site >= w.s0 && site < w.s1 && mac >= min_mac);
        if (lane == 0) qmask[w.blk_off + (b - b0)] = mask;
    }
}

constexpr uint32_t LD_MASK_BATCH = 8;           // masks a thread of the gather loads before it uses them
constexpr uint32_t LD_GATHER_LDS_SITES = 1024;  // the used sites' list lives in LDS up to here, else in the caller's site_list

// grid = windows of the chunk.  qm[2 w] = q, qm[2 w + 1] = m.  site_list: nullptr where max_sites <= LD_GATHER_LDS_SITES, else
// one uint64 per slot of the chunk.  err_bit is ORed into *err when the sites placed are not m.
static __global__ __launch_bounds__(LD_T) void ld_gather_kernel(const uint32_t *__restrict__ sb, const LdWin *__restrict__ wins, uint32_t wps,
                                                                uint32_t G, uint32_t r, const uint32_t *__restrict__ pbits,
                                                                const uint64_t *__restrict__ pos, uint32_t max_sites,
                                                                const uint64_t *__restrict__ qmask, uint32_t *__restrict__ rows,
                                                                uint32_t *__restrict__ cs, uint64_t *__restrict__ coords, uint32_t *__restrict__ qm,
                                                                uint64_t *__restrict__ site_list, uint32_t *__restrict__ err, uint32_t err_bit) {
    __shared__ uint64_t s_site_lds[LD_GATHER_LDS_SITES];
    __shared__ uint32_t s_scan[LD_T];
    __shared__ uint32_t s_placed;
    const uint32_t tid = threadIdx.x;
    const LdWin w = wins[blockIdx.x];
    const uint64_t o = w.row_off;
    const uint32_t cap = w.cap;
    uint64_t *s_site = site_list ? site_list + o : s_site_lds;
    const uint64_t b0 = w.s0 >> 6, nb = w.s1 > w.s0 ? ((w.s1 + 63) >> 6) - b0 : 0;
    const uint64_t *qw = qmask + w.blk_off;
    if (tid == 0) s_placed = 0;
    for (uint32_t k = tid; k < cap; k += LD_T) s_site[k] = w.s0;  // a site that can be read, whatever goes wrong below
    // a thread owns a run of consecutive blocks (one block each up to LD_T blocks, the coalesced case): its count, one exclusive
    // scan over the threads, then the ranks of its blocks' sites in turn.  A chromosome-arm window costs two passes over its
    // masks and one scan, not a scan per LD_T blocks.
    const uint64_t seg = (nb + LD_T - 1) / LD_T;
    const uint64_t i_begin = (uint64_t)tid * seg < nb ? (uint64_t)tid * seg : nb, i_end = i_begin + seg < nb ? i_begin + seg : nb;
    uint32_t mine = 0;
    for (uint64_t i = i_begin; i < i_end; i += LD_MASK_BATCH) {  // a batch of loads in flight, then their counts
        uint64_t v[LD_MASK_BATCH];
#pragma unroll
        for (uint32_t u = 0; u < LD_MASK_BATCH; ++u) v[u] = i + u < i_end ? qw[i + u] : 0ull;
#pragma unroll
        for (uint32_t u = 0; u < LD_MASK_BATCH; ++u) mine += (uint32_t)__popcll(v[u]);
    }
    s_scan[tid] = mine;
    __syncthreads();
    for (uint32_t off = 1; off < LD_T; off <<= 1) {
        const uint32_t v = tid >= off ? s_scan[tid - off] : 0u;
        __syncthreads();
        s_scan[tid] += v;
        __syncthreads();
    }
    const uint64_t q = s_scan[LD_T - 1], m = q < max_sites ? q : max_sites;
    uint64_t rank = (uint64_t)s_scan[tid] - mine;
    uint32_t placed = 0;
    for (uint64_t i = i_begin; i < i_end && m; i += LD_MASK_BATCH) {
        uint64_t v[LD_MASK_BATCH];
#pragma unroll
        for (uint32_t u = 0; u < LD_MASK_BATCH; ++u) v[u] = i + u < i_end ? qw[i + u] : 0ull;
#pragma unroll
        for (uint32_t u = 0; u < LD_MASK_BATCH; ++u) {
            for (uint64_t mask = v[u]; mask; mask &= mask - 1, ++rank) {
                // rank is used iff some k < m has floor(k q / m) == rank; q >= m: at most one, the smallest k >= rank m / q
                const uint64_t k = (rank * m + q - 1) / q;
                if (k < m && k < cap && k * q / m == rank) {
                    s_site[k] = (b0 + i + u) * 64 + (uint64_t)__builtin_ctzll(mask);
                    ++placed;
                }
            }
        }
    }
    if (placed) atomicAdd(&s_placed, placed);
    __syncthreads();
    const uint64_t mc = m < cap ? m : cap;  // m <= cap by the caller's layout; nothing is written past cap if it is not
    for (uint32_t k = tid; k < cap; k += LD_T) coords[o + k] = k < mc ? (pos ? pos[s_site[k]] : s_site[k]) : 0ull;
    uint32_t *dst = rows + o * wps;
    for (uint64_t idx = tid; idx < mc * wps; idx += LD_T) {
        const uint32_t k = (uint32_t)(idx / wps), j = (uint32_t)(idx % wps);
        const uint64_t s = s_site[k];
        dst[idx] = sb[sb_index(wps, G, r, s >> 6, (uint32_t)(s & 63), j)] & pbits[j];
    }
    __syncthreads();  // the rows this workgroup wrote are read back below
    for (uint32_t k = tid; k < mc; k += LD_T) {
        uint32_t c = 0;
        for (uint32_t j = 0; j < wps; ++j) c += __popc(dst[(uint64_t)k * wps + j]);
        cs[o + k] = c;
    }
    if (tid == 0) {
        qm[2 * blockIdx.x] = (uint32_t)q;
        qm[2 * blockIdx.x + 1] = (uint32_t)mc;
        if (s_placed != m || m > cap) atomicOr(err, err_bit);
    }
}

}  // namespace impop
