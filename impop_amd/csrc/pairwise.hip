// pairwise.hip — the all-pairs path: I_ij = sum_s b_is b_js for every haplotype pair of a
// window, then the full pica2 / h-fst semantics (thresholds, rounding,
// greedy grouping) on identities formed on the fly from the integer Gram matrix.
//
// This path is MFMA-bound, not HBM-bound.  Gram kernel: gram_fp4_kernel (FP4 bit planes, below).
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "stats_kernels.h"

namespace impop {

// ---- Gram kernel on the FP4 matrix cores, straight from the raw bit planes (no table, no LDS) ------
// G[i][j] = sum_s x_i[s] x_j[s] as a dense, exact contraction.  One task = one 96 x 96 tile pair (ti <= tj) of one window
// (x one K-slice), owned by one WAVE: 3 x 3 MFMA tiles of 32 x 32 = 144 accumulator registers, which still leaves room for
// TWO waves per SIMD (a lone wave issues one VALU instruction per ~8 cycles, two or more reach one per 2.6 / 4.8 cycles).
// Diagonal tiles reuse A as B and compute only the 6 blocks on and above the block diagonal.
// C/D map of a 32 x 32 block: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).
#ifndef IMPOP_GRAM_ABLATE
#define IMPOP_GRAM_ABLATE 0  // timing-only ablation builds (tools/ablate_gram_fp4.sh): bit 0 no expansion VALU, bit 1 no global loads, bit 3 no result stores
#endif
constexpr int GT = 96;  // tile edge (haplotypes): 3 row groups of 32 (pads 465 haplotypes to 480 instead of 512)

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// v_mfma_f32_32x32x64_f8f6f4 with E2M1 operands runs K = 64 in the 32 cycles the int8 form needs for
// K = 32 (tools/micro/fp4_probe.hip: 8.45 PFLOP/s over the chip), and a 0/1 matrix needs NO table
// for it: the E2M1 nibble 0010 is 1.0, so the four vectors
//     (x << 1) & 0x22222222,  x & 0x22222222,  (x >> 1) & 0x22222222,  (x >> 2) & 0x22222222
// are valid FP4 operands that together hold every bit of the raw dword x exactly once: 7 VALU per 32
// sites of a row.  The four planes of ONE raw
// dword are the four operand dwords of one MFMA (K = 64: lane half 0 supplies 32 sites of cell c,
// lane half 1 the same dword of cell c+1; A and B use the same mapping, so the order of sites inside
// the sum is irrelevant).  fp32 accumulation of 0/1 products is exact below 2^24 (K-slices are
// capped accordingly) and the result is converted to int32 once per task.
// Lane (r = lane & 31, h = lane >> 5) supplies row r of each 32-row group.  RB32: one dwordx2 load of
// a wave = cells c, c+1 of 32 rows = 512 contiguous bytes, and feeds two MFMA phases (dword 0, 1).
// Three cell buffers rotate; a buffer is reloaded right after its last expansion, four phases
// (4 x 9 MFMAs = 1152 cycles) before its next use.
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
struct GramPlanes {          // bit planes of the site weights (weight_planes_kernel), nullptr = unweighted
    const uint32_t *planes;  // plane k at planes + k * stride, one bit per site (dword d = sites 32 d ..)
    uint64_t stride;         // dwords per plane
    uint32_t bits;           // planes with any set bit
};
constexpr uint32_t FP4_MAX_SLICE_PAIRS = (1u << 24) / 128;  // fp32 accumulators stay exact integers

__device__ __forceinline__ i32x4 fp4_planes(uint32_t x) {
    i32x4 f;
    f.x = (int)((x << 1) & 0x22222222u);
    f.y = (int)(x & 0x22222222u);
    f.z = (int)((x >> 1) & 0x22222222u);
    f.w = (int)((x >> 2) & 0x22222222u);
    return f;
}
// the builtin takes 8 dwords per operand; FP4 uses the first 4 (the compiler allocates v[n:n+3])
__device__ __forceinline__ i32x8 fp4_operand(const i32x4 f) { return (i32x8){f.x, f.y, f.z, f.w, 0, 0, 0, 0}; }

typedef int i32x4v __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// A task = tile pair (ti, tj) of a CHAIN of `nchain` windows wins[win0], wins[win0 + wstep], ... (K-slice ks of ksplit; chains
// only with ksplit == 1).  Why chains (round 3): on short windows — a compacted matrix, node-level matrices from a GFA, the
// segments of sliding windows: 2-3 k columns = ~20 pairs = 6 us of MFMAs per task — a task spent more time in its latency chain
// (queue ticket -> window bounds -> first operand loads, each a dependent global round trip) than on the matrix cores.  Inside a
// chain the operand prefetch of the K loop's last iterations reaches into the NEXT window of the chain (same rows, another site
// range: an soffset), and between the weight planes of one window it wraps around to the window's own first pairs, so that only
// the first window of a chain waits for its first loads; one ticket and one scalar load of the bounds per chain link.
template <bool DIAG>
__device__ __forceinline__ void gram_task_fp4(const uint32_t *__restrict__ rb, uint64_t nb_row, uint32_t ti, uint32_t tj,
                                              const GramWindow *__restrict__ wins, uint32_t win0, uint32_t wstep, uint32_t nchain,
                                              uint32_t ks, uint32_t ksplit, int32_t *__restrict__ out, uint64_t out_stride,
                                              uint32_t ld, uint32_t shift, bool add, const GramPlanes wp,
                                              bool out16 /* counts stored as uint16 (host: every window's W < 65536, no atomics) */) {
    constexpr int NB = DIAG ? 0 : 3;
    constexpr int NM = DIAG ? 6 : 9;  // MFMAs per phase
    const uint32_t lane = threadIdx.x & 63, r32 = lane & 31, hi_half = lane >> 5;
    struct Cell {
        u32x2 a[3], b[3];
    };
    struct Frag {  // four FP4 operand dwords per 32-row group, kept as scalars so that asm can define them singly
        uint32_t a[3][4], b[3][4];
    };
    Cell C0, C1, C2;          // raw cells of three consecutive pairs; across chain links they hold the prefetched first pairs
    bool have_cells = false;  // wave-uniform: C0..C2 already hold pairs 0, 1, 2 of the window (plane pass) about to start
    GramWindow w = wins[win0];
    for (uint32_t link = 0; link < nchain; ++link) {
    const uint32_t win = win0 + link * wstep;
    const bool has_next = link + 1 < nchain;
    const GramWindow wn = has_next ? wins[win + wstep] : w;  // next link's bounds, long before the prefetch needs them
    int32_t *__restrict__ o = out16 ? reinterpret_cast<int32_t *>(reinterpret_cast<uint16_t *>(out) + (uint64_t)win * out_stride)
                                    : out + (uint64_t)win * out_stride;
    uint32_t sh = shift;
    bool stored = false;
    // Weighted sites in ONE task (wp.planes != nullptr): I = sum_k 2^k Gram(M & W_k) by Horner over the used bit planes of
    // the weights, highest first — the K loop below runs once per plane with the plane's words ANDed into the A-side mask,
    // the 144 accumulators are doubled in between (exact: powers of two, totals below 2^24) and written ONCE.  One launch
    // per plane instead (operand masked by a separate kernel, (count << k) added into the output) re-wrote the 480^2
    // counts of every window twelve times: 0.9 ms per plane and 2048 node-level windows, most of it output traffic.
    uint32_t plane_left = wp.planes ? wp.bits : 1u;
    uint32_t kcur = 31u - (uint32_t)__builtin_clz(plane_left);
    f32x16 acc[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;
    // entry (row, col) of the tile pair: row = ti*96 + 32a + (e&3) + 8(e>>2) + 4(lane>>5), col = tj*96 + 32b + (lane&31).  The address
    // is a UNIFORM pointer per (a, b, e) (scalar arithmetic) plus ONE per-lane 32-bit offset: 144 per-lane 64-bit addresses would be
    // hoisted out of the chain loop and spilled
    const uint32_t lane_elem = (ti * GT + 4 * (lane >> 5)) * ld + tj * GT + r32;  // < ld^2 <= 2^32 (ld <= 65535 + padding)
    // uint16 counts (half the result bytes: a third of a short-window launch was writing 553 KB of counts per window) go out two
    // to a dword: registers e and e + 1 (e even) of a block are the rows r and r + 1 of this lane's
    // column; a lane swaps both with its neighbour column (DPP quad_perm [1,0,3,2]), even lanes then hold (col, col + 1) of row r,
    // odd lanes (col - 1, col) of row r + 1 — one 4-byte store per lane instead of two 2-byte ones (half the store instructions;
    // on short windows a quarter of the launch was its stores, profiles/r03_gram_experiments.txt §10, §13)
    const uint32_t lane_odd = lane & 1u;
    const uint32_t lane_elem2 = lane_elem + (lane_odd ? ld - 1u : 0u);  // row r + 1, column col - 1 for the odd lanes
    auto store_blocks = [&](int a_from, int a_to) {  // the 32 x 32 blocks of accumulator rows [a_from, a_to) -> int32 counts
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                if (a < a_from || a >= a_to || (DIAG && b < a)) continue;
                if (out16) {
#pragma unroll
                    for (int e = 0; e < 16; e += 2) {
                        const uint64_t eo = (uint64_t)(32 * a + (e & 3) + 8 * (e >> 2)) * ld + 32 * b;  // uniform element offset of (a, b, e)
                        const int32_t v0 = (int32_t)((uint32_t)(int32_t)acc[a][b][e] << sh);
                        const int32_t v1 = (int32_t)((uint32_t)(int32_t)acc[a][b][e + 1] << sh);
                        const int32_t n0 = __builtin_amdgcn_mov_dpp(v0, 0xB1, 0xF, 0xF, true);  // the neighbour column's two rows
                        const int32_t n1 = __builtin_amdgcn_mov_dpp(v1, 0xB1, 0xF, 0xF, true);
                        const uint32_t packed = lane_odd ? (((uint32_t)n1 & 0xFFFFu) | ((uint32_t)v1 << 16))
                                                         : (((uint32_t)v0 & 0xFFFFu) | ((uint32_t)n0 << 16));
                        *reinterpret_cast<uint32_t *>(reinterpret_cast<uint16_t *>(o) + eo + lane_elem2) = packed;
                    }
                    continue;
                }
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const uint64_t eo = (uint64_t)(32 * a + (e & 3) + 8 * (e >> 2)) * ld + 32 * b;  // uniform element offset of (a, b, e)
                    int32_t *ob = o + eo;
                    // weighted matrices: this launch is bit plane `shift` of the site weights, added into the other planes' sum
                    const int32_t v = (int32_t)((uint32_t)(int32_t)acc[a][b][e] << sh);
#if IMPOP_GRAM_ABLATE & 8  // timing-only build: results are not written (only one lane's worth, to keep the work alive)
                    if (lane_elem == 0xFFFFFFFFu) ob[0] = v;
                    continue;
#endif
                    if (ksplit == 1 && !add) ob[lane_elem] = v;
                    else atomicAdd(&ob[lane_elem], v);
                }
            }
    };
    if (w.site_end > w.site_begin) {
        const uint64_t cell0 = w.site_begin >> 6;
        const uint32_t ncell = (uint32_t)(((w.site_end + 63) >> 6) - cell0);
        const uint32_t npair = (ncell + 1) >> 1;  // a pair = cells 2u, 2u+1 (one per lane half) = 128 sites
        const uint32_t ubeg = (uint32_t)((uint64_t)npair * ks / ksplit);
        const uint32_t uend = (uint32_t)((uint64_t)npair * (ks + 1) / ksplit);  // this K-slice: pairs [ubeg, uend)
        const uint32_t f = (uint32_t)((w.site_begin >> 5) - 2 * cell0);           // first window dword (0 or 1)
        const uint32_t l = (uint32_t)(((w.site_end + 31) >> 5) - 1 - 2 * cell0);  // last window dword
        const uint32_t first_mask = 0xFFFFFFFFu << (w.site_begin & 31);
        const uint32_t last_mask = (w.site_end & 31) ? (0xFFFFFFFFu >> (32 - (w.site_end & 31))) : 0xFFFFFFFFu;
        auto mask_of = [&](uint32_t d, bool live) -> uint32_t {  // wave-uniform
            uint32_t m = (live && d >= f && d <= l) ? 0xFFFFFFFFu : 0u;
            if (d == f) m &= first_mask;
            if (d == l) m &= last_mask;
            return m;
        };
        const uint32_t hsel = hi_half ? 0xFFFFFFFFu : 0u;
        auto lane_mask = [&](uint32_t u, int d) -> uint32_t {
            const uint32_t d0 = 4 * u + d;  // dword index of lane half 0 (cell 2u); lane half 1 is one cell (2 dwords) on
            return (hsel & mask_of(d0 + 2, u < uend)) | (~hsel & mask_of(d0, u < uend));
        };
        // the current plane's words for the same two dwords (uniform addresses: scalar loads); past the plane's end the
        // window mask is zero anyway, so the index is only clamped
        const uint32_t *P = nullptr;
        const uint64_t p_lim = wp.planes ? wp.stride - 1 - 2 * cell0 : 0;  // 2 * cell0 < stride: the window starts inside the matrix
        auto plane_mask = [&](uint32_t u, int d) -> uint32_t {
            const uint64_t d0 = 4ull * u + d;
            const uint32_t w0 = P[d0 < p_lim ? d0 : p_lim], w1 = P[d0 + 2 < p_lim ? d0 + 2 : p_lim];
            return (hsel & w1) | (~hsel & w0);
        };
        // Buffer loads: one descriptor per 32-row group, based at the slice's first pair (SGPRs only), the
        // constant per-lane byte offset in voffset and the pair index in soffset: no address VALU at all.
        // (a K-slice is at most FP4_MAX_SLICE_PAIRS * 512 B = 64 MB long, well inside the 32-bit offsets)
        const uint64_t g32b = nb_row * 256;  // bytes between consecutive 32-row groups
        const char *bA = reinterpret_cast<const char *>(rb) + (((uint64_t)(ti * 3) * nb_row + cell0) * 256 + (uint64_t)ubeg * 512);
        const char *bB = reinterpret_cast<const char *>(rb) + (((uint64_t)(tj * 3) * nb_row + cell0) * 256 + (uint64_t)ubeg * 512);
        __amdgpu_buffer_rsrc_t rA[3], rB[3];
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            rA[g] = __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(bA + g * g32b), 0, 0x7FFFFFFF, 0x00020000);
            rB[g] = __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(bB + g * g32b), 0, 0x7FFFFFFF, 0x00020000);
        }
        const uint32_t lane_off = r32 * 8 + hi_half * 256;  // row r32's dword pair inside the lane half's cell
        auto load_one = [&](Cell &C, int i, uint32_t soff) {  // i = 0..2: A groups, 3..5: B groups
            if (i < 3) C.a[i] = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(rA[i], lane_off, soff, 0));
            else C.b[i - 3] = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(rB[i - 3], lane_off, soff, 0));
        };
        // Where the pair loads of the K loop go.  The loop runs n3 = n rounded up to a multiple of 3 pairs (n = uend - ubeg; the
        // filler pairs are fully masked) and loads three pairs ahead, so its last three loads are "pairs" n3, n3 + 1, n3 + 2 into
        // C0, C1, C2: what the NEXT pass starts with — this window's first pairs again if another weight plane follows (`wrap`),
        // else any valid address (the slice's last pair).  The next chain LINK's first pairs are loaded from the store epilogue
        // instead (below): cells alive across all 144 accumulators' stores would not fit the 256 registers of a wave.
        const uint32_t n_pairs = uend - ubeg, n3 = (n_pairs + 2) / 3 * 3;
        bool nx_ok = false;
        uint32_t nx_off = 0, nx_last = 0;  // byte offset of the next link's pair 0 from this slice's descriptor base; its last pair
        if (has_next && ksplit == 1 && wn.site_end > wn.site_begin) {
            const uint64_t cell0n = wn.site_begin >> 6;
            const uint32_t ncelln = (uint32_t)(((wn.site_end + 63) >> 6) - cell0n);
            if (cell0n >= cell0 && (cell0n - cell0) * 256 < 0x7FF00000ull) {
                nx_ok = true;
                nx_off = (uint32_t)((cell0n - cell0) * 256);
                nx_last = ((ncelln + 1) >> 1) - 1;
            }
        }
        bool wrap = false;  // set per plane pass: another plane of this window follows
        auto pair_soff = [&](uint32_t u) -> uint32_t {
            const uint32_t rel = u - ubeg;
            if (rel < n_pairs) return rel * 512u;
            if (rel < n3) return (n_pairs - 1) * 512u;  // masked filler pairs
            const uint32_t j = rel - n3;                // 0, 1, 2
            if (wrap) return (j < n_pairs ? j : n_pairs - 1) * 512u;
            return (n_pairs - 1) * 512u;
        };
        // The phase is scheduled BY HAND in volatile inline asm: builtins let the compiler float the
        // expansion arithmetic across sched_barriers (it is not chained to them) and the MFMAs ended up
        // in runs of 3-9 with the VALU work in one lump behind them.  Volatile asm statements keep their
        // order, so the issue pattern below is the one that runs: MFMA i, then the 4-7 VALU of slot i.
        // Hazards: a fragment register is written >= 7 MFMAs after its last MFMA read and read >= 1 phase
        // after it was written; an accumulator is touched every 9th (6th) MFMA; the compiler cannot see
        // into the asm, so the prologue / epilogue are fenced with explicit s_nop below.
        auto mfma_asm = [](f32x16 &c, const uint32_t (&fa)[4], const uint32_t (&fb)[4]) {
            const i32x4 va = {(int)fa[0], (int)fa[1], (int)fa[2], (int)fa[3]};
            const i32x4 vb = {(int)fb[0], (int)fb[1], (int)fb[2], (int)fb[3]};
            asm volatile("v_mfma_f32_32x32x64_f8f6f4 %0, %1, %2, %0 cbsz:4 blgp:4" : "+v"(c) : "v"(va), "v"(vb));
        };
        auto lo_masked = [](uint32_t (&fr)[4], uint32_t &xm, uint32_t x, uint32_t m) {  // planes 0, 1 of x & m (4 VALU)
            asm volatile("v_and_b32 %2, %3, %4\n\tv_lshlrev_b32 %0, 1, %2\n\tv_and_b32 %0, 0x22222222, %0\n\tv_and_b32 %1, 0x22222222, %2"
                         : "=&v"(fr[0]), "=&v"(fr[1]), "=&v"(xm) : "v"(x), "v"(m));
        };
        auto lo_plain = [](uint32_t (&fr)[4], uint32_t x) {  // planes 0, 1 (3 VALU)
            asm volatile("v_lshlrev_b32 %0, 1, %2\n\tv_and_b32 %0, 0x22222222, %0\n\tv_and_b32 %1, 0x22222222, %2"
                         : "=&v"(fr[0]), "=&v"(fr[1]) : "v"(x));
        };
        auto hi_planes = [](uint32_t (&fr)[4], uint32_t x) {  // planes 2, 3 (4 VALU)
            asm volatile("v_lshrrev_b32 %0, 1, %2\n\tv_and_b32 %0, 0x22222222, %0\n\tv_lshrrev_b32 %1, 2, %2\n\tv_and_b32 %1, 0x22222222, %1"
                         : "=&v"(fr[2]), "=&v"(fr[3]) : "v"(x));
        };
#define FP4_PHASE(CURF, NXTF, SRC, D, M, LOADC, SOFF, DO_LOAD)                                            \
    do {                                                                                                  \
        uint32_t xa0 = 0, xa1 = 0, xa2 = 0;                                                               \
        _Pragma("unroll") for (int i = 0; i < NM; ++i) {                                                  \
            const int a = DIAG ? (i < 3 ? 0 : i < 5 ? 1 : 2) : i / 3;                                     \
            const int b = DIAG ? (i < 3 ? i : i < 5 ? i - 2 : 2) : i % 3;                                 \
            if (DIAG) mfma_asm(acc[a][b], CURF.a[a], CURF.a[b]);                                          \
            else mfma_asm(acc[a][b], CURF.a[a], CURF.b[b]);                                               \
            if (DO_LOAD && !(IMPOP_GRAM_ABLATE & 2) && i < (DIAG ? 3 : 6)) load_one(LOADC, i, SOFF);      \
            if (IMPOP_GRAM_ABLATE & 1) continue; /* timing-only build: no expansion VALU */               \
            if (DIAG) {                                                                                   \
                if (i == 0) lo_masked(NXTF.a[0], xa0, D ? SRC.a[0].y : SRC.a[0].x, M);                    \
                if (i == 1) hi_planes(NXTF.a[0], xa0);                                                    \
                if (i == 2) lo_masked(NXTF.a[1], xa1, D ? SRC.a[1].y : SRC.a[1].x, M);                    \
                if (i == 3) hi_planes(NXTF.a[1], xa1);                                                    \
                if (i == 4) lo_masked(NXTF.a[2], xa2, D ? SRC.a[2].y : SRC.a[2].x, M);                    \
                if (i == 5) hi_planes(NXTF.a[2], xa2);                                                    \
            } else {                                                                                      \
                if (i == 0) lo_masked(NXTF.a[0], xa0, D ? SRC.a[0].y : SRC.a[0].x, M);                    \
                if (i == 1) { hi_planes(NXTF.a[0], xa0); lo_plain(NXTF.b[0], D ? SRC.b[0].y : SRC.b[0].x); } \
                if (i == 2) hi_planes(NXTF.b[0], D ? SRC.b[0].y : SRC.b[0].x);                            \
                if (i == 3) lo_masked(NXTF.a[1], xa1, D ? SRC.a[1].y : SRC.a[1].x, M);                    \
                if (i == 4) { hi_planes(NXTF.a[1], xa1); lo_plain(NXTF.b[1], D ? SRC.b[1].y : SRC.b[1].x); } \
                if (i == 5) hi_planes(NXTF.b[1], D ? SRC.b[1].y : SRC.b[1].x);                            \
                if (i == 6) lo_masked(NXTF.a[2], xa2, D ? SRC.a[2].y : SRC.a[2].x, M);                    \
                if (i == 7) { hi_planes(NXTF.a[2], xa2); lo_plain(NXTF.b[2], D ? SRC.b[2].y : SRC.b[2].x); } \
                if (i == 8) hi_planes(NXTF.b[2], D ? SRC.b[2].y : SRC.b[2].x);                            \
            }                                                                                             \
        }                                                                                                 \
    } while (0)
        // pair U lives in CUR (its dword 0 is already expanded in F); NXT holds pair U+1.  The mask
        // arithmetic sits behind a wave-uniform branch that only edge pairs take (the empty volatile asm
        // keeps the compiler from turning it back into always-executed selects); the MFMA code is common.
#define FP4_PAIR(CUR, NXT, U)                                                       \
    do {                                                                            \
        uint32_t mA = 0xFFFFFFFFu, mB = 0xFFFFFFFFu;                                \
        if (!(4 * (U) + 1 > f && 4 * (U) + 6 < l && (U) + 1 < uend)) {              \
            asm volatile("");                                                       \
            mA = lane_mask((U), 1);                                                 \
            mB = lane_mask((U) + 1, 0);                                             \
        }                                                                           \
        if (P) {                                                                    \
            mA &= plane_mask((U), 1);                                               \
            mB &= plane_mask((U) + 1, 0);                                           \
        }                                                                           \
        const uint32_t soff = pair_soff((U) + 3);                                   \
        FP4_PHASE(F, G, CUR, 1, mA, CUR, soff, false);                              \
        FP4_PHASE(G, F, NXT, 0, mB, CUR, soff, true);                               \
    } while (0)
        do {  // once, or once per used weight plane (a plain bottom-tested loop: more exits make the compiler shuffle the accumulators)
        if (wp.planes) P = wp.planes + (uint64_t)kcur * wp.stride + 2 * cell0;
        if (ubeg < uend) {
            Frag F, G;
            wrap = (plane_left & ~(1u << kcur)) != 0;
            if (!have_cells) {  // first link of a chain (or nothing could be prefetched): wait for the first three pairs here
#pragma unroll
                for (int i = 0; i < (DIAG ? 3 : 6); ++i) {
                    load_one(C0, i, pair_soff(ubeg));
                    load_one(C1, i, pair_soff(ubeg + 1));
                    load_one(C2, i, pair_soff(ubeg + 2));
                }
            }
            have_cells = wrap;  // what the loop below leaves in C0..C2 (pair_soff)
            {
                const uint32_t m0 = lane_mask(ubeg, 0) & (P ? plane_mask(ubeg, 0) : 0xFFFFFFFFu);
                uint32_t xm;
#pragma unroll
                for (int g = 0; g < 3; ++g) {
                    lo_masked(F.a[g], xm, C0.a[g].x, m0);
                    hi_planes(F.a[g], xm);
                }
#pragma unroll
                for (int g = 0; g < NB; ++g) {
                    lo_plain(F.b[g], C0.b[g].x);
                    hi_planes(F.b[g], C0.b[g].x);
                }
#if IMPOP_GRAM_ABLATE & 1  // timing-only build without the in-loop expansion: G needs realistic contents too
#pragma unroll
                for (int g = 0; g < 3; ++g) {
                    lo_masked(G.a[g], xm, C1.a[g].y, m0);
                    hi_planes(G.a[g], xm);
                }
#pragma unroll
                for (int g = 0; g < NB; ++g) {
                    lo_plain(G.b[g], C1.b[g].y);
                    hi_planes(G.b[g], C1.b[g].y);
                }
#endif
                asm volatile("s_nop 7");  // VALU-written operands -> first MFMA (the compiler cannot see into the asm)
            }
            // no early exit (extra loop exits make the compiler merge 144 accumulators and spill): a slice
            // whose length is not a multiple of 3 pairs runs up to two fully masked pairs
            for (uint32_t u = ubeg; u < uend; u += 3) {
                FP4_PAIR(C0, C1, u);
                FP4_PAIR(C1, C2, u + 1);
                FP4_PAIR(C2, C0, u + 2);
            }
        }
        asm volatile("s_nop 15\n\ts_nop 15");  // last MFMA results -> the VALU conversions / doublings below
        plane_left &= ~(1u << kcur);
        const uint32_t knext = plane_left ? 31u - (uint32_t)__builtin_clz(plane_left) : kcur;
        const float up = (float)(1u << (kcur - knext));  // planes without a set bit in between are skipped; x1 after the last
        kcur = knext;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                if (DIAG && b < a) continue;
                acc[a][b] *= up;
            }
        asm volatile("s_nop 7");  // VALU-written accumulators -> the next plane's first MFMA
        } while (plane_left);
        // results out; the next chain link's first three pairs are requested once the first row of accumulator blocks has gone
        // (its registers are free by then), so their latency runs under the other two thirds of the stores and the next link's set-up
        if (wp.planes) sh += kcur;  // Horner stopped at the lowest used plane
        store_blocks(0, 1);
        __builtin_amdgcn_sched_barrier(0);  // the loads stay HERE: hoisted above the stores they would not fit the registers
        if (nx_ok) {
#pragma unroll
            for (int i = 0; i < (DIAG ? 3 : 6); ++i) {
                load_one(C0, i, nx_off);
                load_one(C1, i, nx_off + (1 < nx_last ? 1 : nx_last) * 512u);
                load_one(C2, i, nx_off + (2 < nx_last ? 2 : nx_last) * 512u);
            }
            have_cells = true;
        }
        __builtin_amdgcn_sched_barrier(0);
        store_blocks(1, 3);
        stored = true;
#undef FP4_PAIR
#undef FP4_PHASE
    }
    if (!stored) store_blocks(0, 3);  // an empty window never started: zeros
    w = wn;
    }  // chain links
}

// Persistent workgroups (2 per CU, 4 waves each, no LDS); every WAVE pulls (window, tile pair, K-slice) tasks from one of 8
// queues until all are drained, so a wave whose task was short (diagonal tiles do 2/3 of the MFMAs) immediately starts another
// one and both SIMD slots stay occupied (PMC before queues: 1.45-1.6 resident waves per SIMD, after: ~2).
// Queue q holds the tasks of windows with win % 8 == q and is served first by workgroups with blockIdx % 8 == q, i.e. (under
// the observed round-robin placement) by one XCD, whose L2 then holds that window's rows for all of its 15 tile pairs; a
// workgroup whose queue is empty steals from the others, so the result and termination never depend on placement: every wave
// leaves once all eight counters have passed their queue length.
// ksplit > 1: the site range of a window is cut into ksplit slices handled by different tasks that atomicAdd into a
// zero-initialised output (integer adds commute: still bit-reproducible); used when there are too few (window, tile) tasks to
// keep two waves on every SIMD.
__global__ __launch_bounds__(256, 2) void gram_fp4_kernel(const uint32_t *__restrict__ rb, uint64_t nb_row, uint32_t n_tiles,
                                                          uint32_t tasks_per_win, uint32_t n_win, uint32_t ksplit,
                                                          const GramWindow *__restrict__ wins, int32_t *__restrict__ out,
                                                          uint32_t ld, uint64_t out_stride, uint32_t *__restrict__ queue_heads,
                                                          uint32_t shift, bool add, GramPlanes wp, uint32_t chain, uint32_t out16) {
    const uint32_t slots = tasks_per_win * ksplit;  // (tile pair, K-slice) slots of one window
    const bool by_window = n_win >= 8;              // few windows: deal single tasks round-robin instead
    const uint64_t total = (uint64_t)n_win * slots;
    const uint32_t nc = (by_window && ksplit == 1 && chain > 1) ? chain : 1u;  // windows per ticket (gram_task_fp4: chains)
    for (uint32_t dq = 0; dq < 8; ++dq) {
        const uint32_t q = (blockIdx.x + dq) & 7;
        const uint32_t nwq = (n_win + 7 - q) / 8;  // windows of queue q: q, q + 8, ...
        const uint64_t q_len = by_window ? (uint64_t)((nwq + nc - 1) / nc) * slots : (total + 7 - q) / 8;
        for (;;) {
            uint32_t k = 0;
            if ((threadIdx.x & 63) == 0) k = atomicAdd(&queue_heads[q], 1u);
            k = __builtin_amdgcn_readfirstlane(k);
            if (k >= q_len) break;  // queue drained (the head keeps counting, harmlessly)
            uint32_t win, t2, links = 1, wstep = 0;
            if (by_window) {
                const uint32_t wb = k / slots;  // ticket = (block of nc windows of this queue, tile pair)
                t2 = k % slots;
                win = q + 8 * (wb * nc);
                links = nwq - wb * nc < nc ? nwq - wb * nc : nc;
                wstep = 8;
            } else { const uint64_t i = q + 8ull * k; win = (uint32_t)(i / slots); t2 = (uint32_t)(i % slots); }
            const uint32_t ks = t2 % ksplit;
            uint32_t rem = t2 / ksplit, ti = 0, tj;
            while (rem >= n_tiles - ti) { rem -= n_tiles - ti; ++ti; }
            tj = ti + rem;
            if (ti == tj) gram_task_fp4<true>(rb, nb_row, ti, tj, wins, win, wstep, links, ks, ksplit, out, out_stride, ld, shift, add, wp, out16 != 0);
            else gram_task_fp4<false>(rb, nb_row, ti, tj, wins, win, wstep, links, ks, ksplit, out, out_stride, ld, shift, add, wp, out16 != 0);
        }
    }
}

// The operand is stored in minor-allele polarity (layout.hip sb_to_hm_kernel; m->phi_row): the counts the Gram kernel wrote are
// I'_ij of the stored bits, with row / column p = phi_row holding I'_ip = (complemented sites haplotype i is stored with a 1 at)
// and I'_pp = the number of complemented sites (weights: their summed weights).  For a complemented site b = 1 - b', so
//     I_ij = I'_ij + I'_pp - I'_ip - I'_jp          (i <= j < n; the diagonal a_i = I_ii likewise)
// Exact integers.  Needed where I or a themselves matter — the `dice` identity, exported counts; the `match` identity and every
// statistic built on it see only a_i + a_j - 2 I_ij, which is the same in both polarities, and skip this pass.
// grid: (matrices, row chunks); dynamic LDS: n int32.
template <typename T>  // int32_t, or uint16_t (counts of short windows, SimBatch.g16)
__global__ __launch_bounds__(256) void gram_unflip_kernel(T *__restrict__ g, uint32_t ld, uint64_t stride, uint32_t n, uint32_t phi) {
    extern __shared__ int32_t unflip_t[];
    T *G = g + (uint64_t)blockIdx.x * stride;
    for (uint32_t i = threadIdx.x; i < n; i += 256) unflip_t[i] = (int32_t)G[(uint64_t)i * ld + phi];
    const int32_t P = (int32_t)G[(uint64_t)phi * ld + phi];
    __syncthreads();
    for (uint32_t i = blockIdx.y; i < n; i += gridDim.y) {
        const int32_t ri = P - unflip_t[i];
        T *row = G + (uint64_t)i * ld;
        for (uint32_t j = i + threadIdx.x; j < n; j += 256) row[j] = (T)((int32_t)row[j] + ri - unflip_t[j]);  // column phi itself (j = n) stays as written
    }
}
int launch_gram_unflip(impop_ctx *ctx, const impop_matrix *m, int32_t *d_g, uint64_t n_mats, bool g16) {
    if (m->phi_row == 0xFFFFFFFFu || n_mats == 0) return IMPOP_OK;
    const uint32_t n = m->g.n_hap, ld = m->n_hap_pad;
    REQUIRE(n_mats < 0x7FFFFFFFull && (size_t)n * 4 <= 64 * 1024, "gram_unflip: too many matrices / haplotypes");
    const uint32_t chunks = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(4096 / n_mats, 1), 64);
    if (g16)
        hipLaunchKernelGGL(gram_unflip_kernel<uint16_t>, dim3((uint32_t)n_mats, chunks), dim3(256), (size_t)n * 4, ctx->stream,
                           reinterpret_cast<uint16_t *>(d_g), ld, (uint64_t)ld * ld, n, m->phi_row);
    else
        hipLaunchKernelGGL(gram_unflip_kernel<int32_t>, dim3((uint32_t)n_mats, chunks), dim3(256), (size_t)n * 4, ctx->stream, d_g, ld,
                           (uint64_t)ld * ld, n, m->phi_row);
    HIP_TRY(hipGetLastError());
    return IMPOP_OK;
}

// mirror the upper tiles into the lower triangle (only for host export)
__global__ void gram_symmetrize_kernel(int32_t *g, uint32_t ld) {
    const uint32_t i = blockIdx.y * blockDim.y + threadIdx.y, j = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < ld && j < ld && i > j) g[(uint64_t)i * ld + j] = g[(uint64_t)j * ld + i];
}

__global__ void identity_dense_kernel(SimBatch b, uint32_t n, double *__restrict__ out) {
    const uint32_t i = blockIdx.y * blockDim.y + threadIdx.y, j = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || j >= n) return;
    const SimView S = sim_view(b, 0);
    out[(uint64_t)i * n + j] = sim_get(S, i, j);
}

// add_shift < 0: d_out = Gram; >= 0: d_out += Gram << add_shift (d_out holds the other planes' sum).
// fused_planes: the weighted Gram matrix of m in one launch (gram_task_fp4), every window's summed weight below 2^24.
// out16 (in / out, nullable): the caller would take uint16 counts (every window's W < 65536); set to whether the launch wrote them
// (only without K-split atomics and plane accumulation)
static int launch_gram(impop_ctx *ctx, const impop_matrix *m, const uint32_t *d_rb, const GramWindow *d_wins, uint32_t n_win,
                       int32_t *d_out, uint64_t max_window_sites, int add_shift = -1, bool fused_planes = false, bool *out16 = nullptr) {
    const uint32_t T = m->n_hap_pad / GT;
    const uint32_t tasks_per_win = T * (T + 1) / 2;  // upper-triangular tile pairs
    // two waves per SIMD on every CU = 8 * n_cu resident waves; aim at >= 4 rounds of them so the
    // last, partially filled round does not dominate, and split the site axis when there are fewer tasks
    const uint64_t want = 32ull * (uint64_t)(ctx->n_cu > 0 ? ctx->n_cu : 256);
    uint32_t ksplit = 1;
    while ((uint64_t)n_win * tasks_per_win * ksplit < want && ksplit < 64) ksplit *= 2;
    // fp32 accumulators must stay below 2^24 per K-slice
    while ((max_window_sites / 128 + 2) / ksplit + 1 > FP4_MAX_SLICE_PAIRS) ksplit *= 2;
    const bool w16 = out16 && *out16 && ksplit == 1 && add_shift < 0;
    if (out16) *out16 = w16;
    if (ksplit > 1 && add_shift < 0)
        HIP_TRY(hipMemsetAsync(d_out, 0, (size_t)n_win * m->n_hap_pad * m->n_hap_pad * sizeof(int32_t), ctx->stream));
    REQUIRE((uint64_t)n_win * tasks_per_win * ksplit < 0xFFFFFFF0ull, "gram: too many tasks for one launch");
    if (!ctx->d_queue) HIP_TRY(hipMalloc((void **)&ctx->d_queue, 8 * sizeof(uint32_t)));
    HIP_TRY(hipMemsetAsync(ctx->d_queue, 0, 8 * sizeof(uint32_t), ctx->stream));
    // persistent grid: two 256-thread workgroups per CU, never fewer than 8
    const uint32_t n_cu = (uint32_t)(ctx->n_cu > 0 ? ctx->n_cu : 256);
    const uint64_t need_wg = ((uint64_t)n_win * tasks_per_win * ksplit + 3) / 4;
    const uint32_t grid = (uint32_t)std::max<uint64_t>(8, std::min<uint64_t>(2ull * n_cu, need_wg));
    GramPlanes wp{nullptr, 0, 0};
    if (fused_planes) wp = GramPlanes{m->d_wplanes, m->wplane_stride, m->wplane_bits};
    // chains of windows per ticket (gram_task_fp4) where a task is short — at most 8192 columns = 64 pairs, 20 us of MFMAs — and
    // there are enough tasks that every wave still draws >= 4 tickets (so the grid's last round stays small); IMPOP_GRAM_CHAIN=n overrides
    uint32_t chain = 1;
    const uint64_t planes_walked = fused_planes ? std::max<uint32_t>((uint32_t)__builtin_popcount(m->wplane_bits), 1u) : 1u;  // K passes per window
    if (ksplit == 1 && n_win >= 8 && max_window_sites * planes_walked <= 8192) {
        const uint64_t per_wave = (uint64_t)n_win * tasks_per_win / (8ull * n_cu);
        chain = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(per_wave / 4, 1), 8);  // measured (tools/ab_chain.py): 1.90 / 1.79 / 1.75 ms
    }                                                                                  // per 4096 compacted windows at 1 / 3 / 8 links
    {
        static const int forced = [] { const char *e = getenv("IMPOP_GRAM_CHAIN"); return e ? atoi(e) : 0; }();
        if (forced > 0 && ksplit == 1) chain = (uint32_t)forced;
    }
    {  // IMPOP_TRACE=1: the launch configuration (the chain as gram_fp4_kernel applies it: only with >= 8 cells and no K-split)
        if (trace_on())
            fprintf(stderr, "[impop_gram] cells=%u tiles=%u ksplit=%u chain=%u u16=%d fused_planes=%d\n", n_win, T, ksplit,
                    (n_win >= 8 && ksplit == 1) ? chain : 1u, w16 ? 1 : 0, fused_planes ? 1 : 0);
    }
    hipLaunchKernelGGL(gram_fp4_kernel, dim3(grid), dim3(256), 0, ctx->stream, d_rb, m->rb_nb, T, tasks_per_win, n_win, ksplit,
                       d_wins, d_out, m->n_hap_pad, (uint64_t)m->n_hap_pad * m->n_hap_pad, ctx->d_queue,
                       add_shift < 0 ? 0u : (uint32_t)add_shift, add_shift >= 0, wp, chain, w16 ? 1u : 0u);
    HIP_TRY(hipGetLastError());
    return IMPOP_OK;
}

// every window lighter than 2^24 (fp32-exact sums): all weight planes inside one launch (Horner in gram_task_fp4)
constexpr uint64_t GRAM_FUSED_WEIGHT_LIMIT = 1ull << 24;

// ---- weighted sites on the all-pairs path ------------------------------------------------------------------
// Column s stands for w_s base pairs (one column per graph node, impop_matrix_set_site_weights): what `impg
// similarity` hands the reference is a bp-weighted node-sharing identity (run_pica2_impg.sh:162-175), i.e.
//     I_ij = sum_s w_s b_is b_js.
// Write w_s = sum_k 2^k w_ks with bit planes w_ks in {0,1}.  Masking the site axis with plane k gives a 0/1
// matrix M_k = M & W_k whose plain Gram matrix is sum_s w_ks b_is b_js (w_ks^2 = w_ks), so
//     I = sum_k 2^k Gram(M_k)
// with the same matrix-core pipeline.  Usual case (every window lighter than 2^24): ONE launch, the planes walked inside
// each task (gram_task_fp4, GramPlanes).  Otherwise, per plane, one elementwise AND of the RB32 operand (only the cells
// the batch touches) and one Gram launch whose epilogue ADDS (count << k) into the sum of the planes before it (integer
// atomics; a separate shifted-accumulate pass over 4096 x 480^2 counts cost 1.0 ms per plane, twice the Gram launch it
// followed).  tools/bench_weighted.py, 4096 node-level windows of 12 planes: 46 ms (separate pass) -> 30 ms (epilogue
// adds) -> 8.3 ms (planes in the task).  Exact by construction (every partial Gram is an exact integer; the sum is required
// to stay below 2^31 like the length of an unweighted window); planes without any set bit are skipped, so node lengths
// below 2^p cost p passes over the NODE-level matrix — against mean-node-length times the MACs for the bp-expanded one.
__global__ void weight_planes_kernel(const uint32_t *__restrict__ wt, uint64_t n_site, uint64_t n_dword, uint32_t n_plane,
                                     uint32_t *__restrict__ planes, uint32_t *__restrict__ used_bits) {
    const uint64_t d = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= n_dword) return;
    uint32_t any = 0;
    uint32_t w[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        const uint64_t s = 32 * d + j;
        w[j] = s < n_site ? wt[s] : 0u;
        any |= w[j];
    }
    for (uint32_t k = 0; k < n_plane; ++k) {
        uint32_t bits = 0;
#pragma unroll
        for (int j = 0; j < 32; ++j) bits |= ((w[j] >> k) & 1u) << j;
        planes[(uint64_t)k * n_dword + d] = bits;
    }
    if (any) atomicOr(used_bits, any);
}

// masked operand for plane k over the cells [cell_lo, cell_hi) of every 32-row group (one thread = one row's dword pair)
__global__ void rb_mask_kernel(const uint32_t *__restrict__ rb, uint32_t *__restrict__ out, uint64_t rb_nb, uint32_t n_group,
                               uint64_t cell_lo, uint64_t cell_hi, const uint32_t *__restrict__ plane, uint64_t n_dword) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t per_group = (cell_hi - cell_lo) * 32;
    if (t >= per_group * n_group) return;
    const uint64_t g = t / per_group, r = t % per_group, cell = cell_lo + r / 32;
    const uint64_t at = ((g * rb_nb + cell) * 32 + (r & 31)) * 2;
    const u32x2 v = *reinterpret_cast<const u32x2 *>(rb + at);
    u32x2 o;
    o.x = 2 * cell < n_dword ? v.x & plane[2 * cell] : 0u;
    o.y = 2 * cell + 1 < n_dword ? v.y & plane[2 * cell + 1] : 0u;
    *reinterpret_cast<u32x2 *>(out + at) = o;
}

static int ensure_weight_planes(impop_ctx *ctx, const impop_matrix *m) {
    if (m->d_wplanes) return IMPOP_OK;
    const uint64_t n_dword = 2 * m->g.n_block;
    if (n_dword == 0) {  // no column at all (a weighted matrix compacted to nothing): no plane has a bit
        m->wplane_bits = 0;
        m->wplane_stride = 0;
        return IMPOP_OK;
    }
    uint32_t *d_used = nullptr;
    HIP_TRY(hipMalloc((void **)&m->d_wplanes, 32ull * n_dword * 4 + 256));
    d_used = m->d_wplanes + 32ull * n_dword;
    HIP_TRY(hipMemsetAsync(d_used, 0, 4, ctx->stream));
    hipLaunchKernelGGL(weight_planes_kernel, dim3((uint32_t)((n_dword + 127) / 128)), dim3(128), 0, ctx->stream, m->d_wt, m->g.n_site,
                       n_dword, 32u, m->d_wplanes, d_used);
    HIP_TRY(hipGetLastError());
    uint32_t used = 0;
    HIP_TRY(hipMemcpyAsync(&used, d_used, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    m->wplane_bits = used;
    m->wplane_stride = n_dword;
    if (!m->d_rb_masked) HIP_TRY(hipMalloc((void **)&m->d_rb_masked, m->rb_bytes));
    return IMPOP_OK;
}

// Gram matrices of `n_win` cells (host copy h_wins of d_wins for the cell range) into d_out
int launch_gram_any(impop_ctx *ctx, const impop_matrix *m, const GramWindow *d_wins, const GramWindow *h_wins, uint32_t n_win,
                    int32_t *d_out, uint64_t max_window_sites, bool *out16) {
    if (m->wt_prefix.empty()) return launch_gram(ctx, m, m->d_rb, d_wins, n_win, d_out, max_window_sites, -1, false, out16);
    int rc = ensure_weight_planes(ctx, m);
    if (rc) return rc;
    uint64_t c_lo = ~0ull, c_hi = 0;
    for (uint32_t i = 0; i < n_win; ++i)
        if (h_wins[i].site_end > h_wins[i].site_begin) {
            c_lo = std::min(c_lo, h_wins[i].site_begin >> 6);
            c_hi = std::max(c_hi, (h_wins[i].site_end + 63) >> 6);
        }
    const uint64_t count = (uint64_t)n_win * m->n_hap_pad * m->n_hap_pad;
    uint64_t heaviest = 0;
    const std::vector<uint64_t> &pre = m->compact ? m->kept_wt_prefix : m->wt_prefix;  // the cells are in MATRIX coordinates
    for (uint32_t i = 0; i < n_win; ++i)
        if (h_wins[i].site_end > h_wins[i].site_begin)
            heaviest = std::max(heaviest, pre[h_wins[i].site_end] - pre[h_wins[i].site_begin]);
    if (m->wplane_bits && heaviest < GRAM_FUSED_WEIGHT_LIMIT) {
        if (out16 && heaviest >= 65536) *out16 = false;
        return launch_gram(ctx, m, m->d_rb, d_wins, n_win, d_out, max_window_sites, -1, true, out16);
    }
    if (out16) *out16 = false;  // one launch per plane, accumulated with atomics: 32-bit counts
    HIP_TRY(hipMemsetAsync(d_out, 0, count * 4, ctx->stream));
    if (c_lo >= c_hi) return IMPOP_OK;
    c_hi = std::min<uint64_t>(c_hi + 8, m->rb_nb);  // the Gram pipeline prefetches a few cells past a window's end
    const uint32_t n_group = m->n_hap_pad / 32;
    const uint64_t threads = (c_hi - c_lo) * 32 * n_group;
    REQUIRE((threads + 255) / 256 < 0x7FFFFFFFull, "weighted Gram: batch too large");
    for (uint32_t k = 0; k < 32; ++k) {
        if (!((m->wplane_bits >> k) & 1u)) continue;
        hipLaunchKernelGGL(rb_mask_kernel, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, ctx->stream, m->d_rb, m->d_rb_masked,
                           m->rb_nb, n_group, c_lo, c_hi, m->d_wplanes + (uint64_t)k * m->wplane_stride, m->wplane_stride);
        HIP_TRY(hipGetLastError());
        // the plane's shift and the sum over planes happen in the Gram kernel's own stores
        rc = launch_gram(ctx, m, m->d_rb_masked, d_wins, n_win, d_out, max_window_sites, (int)k);
        if (rc) return rc;
    }
    return IMPOP_OK;
}

// ---- S for the all-pairs path from a cached site bitmap -----------------------------------------------------------
// S = #{s in window : 0 < c_s < n} (all haplotypes: run_tajd.sh:126,148 take S from the un-subset graph).  Whether a
// site segregates does not depend on the window, so it is computed ONCE per matrix — one streaming pass over the
// SB64 layout, one bit per site — and kept with the matrix; a window's S is then a popcount over W / 8 bytes
// instead of a second pass over its n W / 8 bytes behind every Gram launch (that pass was 1.83 ms of every
// 12 ms batch of 4096 windows; the first call on a matrix still pays it once).
typedef uint32_t u32q __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void segmap_kernel(const uint32_t *__restrict__ sb, uint32_t wps, uint32_t G, uint32_t r, uint32_t n,
                                                     uint64_t n_block, uint32_t *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t b = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= n_block) return;  // wave-uniform
    const uint32_t *blk = sb + b * 64ull * wps;
    uint32_t c = 0;
    for (uint32_t g = 0; g + 1 < G; ++g) {
        const u32q v = __builtin_nontemporal_load(reinterpret_cast<const u32q *>(blk + (uint64_t)g * 256 + lane * 4));
        c += __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
    }
    for (uint32_t e = 0; e < r; ++e) c += __popc(__builtin_nontemporal_load(blk + (uint64_t)(G - 1) * 256 + lane * r + e));
    const uint64_t bal = __ballot((c - 1u) < (n - 1u));  // padding sites of the last block are all-zero: not segregating
    if (lane == 0) { out[2 * b] = (uint32_t)bal; out[2 * b + 1] = (uint32_t)(bal >> 32); }
}

// one wave per window: popcount of the bitmap over [site_begin, site_end) -> s_all and s_p of the window's record
__global__ __launch_bounds__(256) void seg_count_kernel(const uint32_t *__restrict__ map, const GramWindow *__restrict__ wins,
                                                        uint64_t n_win, impop_window_stats *__restrict__ stats /* nullable */,
                                                        uint32_t *__restrict__ plain /* nullable: one count per window */) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t w = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= n_win) return;
    const uint64_t s0 = wins[w].site_begin, s1 = wins[w].site_end;
    const uint64_t d0 = s0 >> 5, d1 = (s1 + 31) >> 5;
    uint32_t cnt = 0;
    for (uint64_t d = d0 + lane; d < d1; d += 64) {
        uint32_t v = map[d];
        if (d == d0) v &= 0xFFFFFFFFu << (s0 & 31);
        if (d == d1 - 1 && (s1 & 31)) v &= 0xFFFFFFFFu >> (32 - (s1 & 31));
        cnt += __popc(v);
    }
    cnt = wave_sum_u32(cnt);
    if (lane == 0) {
        if (stats) { stats[w].s_all = cnt; stats[w].s_p = cnt; }
        if (plain) plain[w] = cnt;
    }
}

// compacted matrix: the dropped all-ones sites of [site_begin, site_end) (ORIGINAL coordinates) add 1 to every I_ij
__global__ void gram_add_const_kernel(int32_t *__restrict__ g, uint32_t ld, uint32_t n, const uint32_t *__restrict__ add) {
    const uint32_t i = blockIdx.y * blockDim.y + threadIdx.y, j = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && j < n) g[(uint64_t)i * ld + j] += (int32_t)add[0];
}

// kept-site index range of an original-coordinate range on a compacted matrix (identity otherwise)
static inline void map_range(const impop_matrix *m, uint64_t s0, uint64_t s1, uint64_t *k0, uint64_t *k1) {
    if (!m->compact) { *k0 = s0; *k1 = s1; return; }
    *k0 = pos_lower_bound(m, s0);
    *k1 = pos_lower_bound(m, s1);
}

int ensure_segmap(impop_ctx *ctx, const impop_matrix *m) {
    if (m->d_segmap || m->g.n_block == 0) return IMPOP_OK;
    HIP_TRY(hipMalloc((void **)&m->d_segmap, m->g.n_block * 8 + 256));
    REQUIRE((m->g.n_block + 3) / 4 < 0x7FFFFFFFull, "site bitmap: matrix too long for one launch");
    hipLaunchKernelGGL(segmap_kernel, dim3((uint32_t)((m->g.n_block + 3) / 4)), dim3(256), 0, ctx->stream, m->d_sb, m->g.wps, m->g.G,
                       m->g.r, m->g.n_hap, m->g.n_block, m->d_segmap);
    HIP_TRY(hipGetLastError());
    return IMPOP_OK;
}

int launch_seg_count(impop_ctx *ctx, const uint32_t *d_map, const GramWindow *d_wins, uint64_t n_win, impop_window_stats *d_stats,
                     uint32_t *d_plain) {
    hipLaunchKernelGGL(seg_count_kernel, dim3((uint32_t)((n_win + 3) / 4)), dim3(256), 0, ctx->stream, d_map, d_wins, n_win, d_stats, d_plain);
    HIP_TRY(hipGetLastError());
    return IMPOP_OK;
}

int check_pairwise_args(impop_ctx *ctx, const impop_matrix *m, uint64_t s0, uint64_t s1, const char *fn) {
    REQUIRE(ctx && m, "%s: NULL argument", fn);
    if (m->compact && !(m->d_rb && m->d_onesmap)) {
        set_error("%s: this compacted matrix has no all-pairs operand (compact a matrix that kept IMPOP_KEEP_HAP_MAJOR)", fn);
        return IMPOP_E_UNSUPPORTED;
    }
    REQUIRE(m->d_rb, "%s: matrix was created without IMPOP_KEEP_HAP_MAJOR", fn);
    REQUIRE(s0 <= s1 && s1 <= matrix_span(m), "%s: bad site range [%llu,%llu)", fn, (unsigned long long)s0,
            (unsigned long long)s1);
    REQUIRE(window_W(m, s0, s1) < (1ull << 31), "%s: window of 2^31 or more sites (or summed site weights) overflows int32 counts", fn);
    return IMPOP_OK;
}

// The Gram matrix of ONE window [s0, s1) (original coordinates), in the original polarity, for the calls that export counts or
// identities: scratch for L's sub-buffers (the caller's own, listed before the call) plus the helper's, the window mapped and
// uploaded, the Gram launch, the unflip; *d_g = the ld x ld counts.  Compacted matrix: *d_add = the constant every I_ij lacks —
// the dropped sites every haplotype carries (their count, or their summed weights) — else nullptr.
static int gram_one_window(impop_ctx *ctx, const impop_matrix *m, uint64_t s0, uint64_t s1, Layout &L, int32_t **d_g, uint32_t **d_add) {
    const uint32_t ld = m->n_hap_pad;
    GramWindow *d_w, *d_ow;
    uint32_t *d_a;
    L.sub(d_w, 1); L.sub(*d_g, (size_t)ld * ld); L.sub(d_ow, 1); L.sub(d_a, 1);
    void *d = nullptr;
    int rc = ctx_scratch(ctx, L.total(), &d);
    if (rc) return rc;
    L.bind(d);
    GramWindow w;
    map_range(m, s0, s1, &w.site_begin, &w.site_end);  // compacted: the kept sites of the range
    HIP_TRY(hipMemcpyAsync(d_w, &w, sizeof w, hipMemcpyHostToDevice, ctx->stream));
    rc = launch_gram_any(ctx, m, d_w, &w, 1, *d_g, w.site_end - w.site_begin);
    if (rc) return rc;
    rc = launch_gram_unflip(ctx, m, *d_g, 1);
    if (rc) return rc;
    *d_add = m->compact ? d_a : nullptr;
    if (compact_weighted(m)) {
        const uint32_t add_w = ones_weight(m, s0, s1);
        HIP_TRY(hipMemcpyAsync(d_a, &add_w, 4, hipMemcpyHostToDevice, ctx->stream));
    } else if (m->compact) {
        const GramWindow ow{s0, s1};
        HIP_TRY(hipMemcpyAsync(d_ow, &ow, sizeof ow, hipMemcpyHostToDevice, ctx->stream));
        rc = launch_seg_count(ctx, m->d_onesmap, d_ow, 1, nullptr, d_a);
    }
    return rc;
}

}  // namespace impop

using namespace impop;

IMPOP_API int impop_pairwise_counts(impop_ctx *ctx, const impop_matrix *m, uint64_t site_begin, uint64_t site_end,
                                    int32_t *out_host) {
    int rc = check_pairwise_args(ctx, m, site_begin, site_end, "impop_pairwise_counts");
    if (rc) return rc;
    REQUIRE(out_host, "impop_pairwise_counts: out is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    const uint32_t n = m->g.n_hap, ld = m->n_hap_pad;
    Layout L;
    int32_t *d_g;
    uint32_t *d_add;
    rc = gram_one_window(ctx, m, site_begin, site_end, L, &d_g, &d_add);
    if (rc) return rc;
    if (d_add) {
        hipLaunchKernelGGL(gram_add_const_kernel, dim3((n + 15) / 16, (n + 15) / 16), dim3(16, 16), 0, ctx->stream, d_g, ld, n, d_add);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(gram_symmetrize_kernel, dim3((ld + 15) / 16, (ld + 15) / 16), dim3(16, 16), 0, ctx->stream, d_g, ld);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy2DAsync(out_host, (size_t)n * 4, d_g, (size_t)ld * 4, (size_t)n * 4, n, hipMemcpyDeviceToHost,
                             ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return IMPOP_OK;
}

IMPOP_API int impop_pairwise_identity(impop_ctx *ctx, const impop_matrix *m, uint64_t site_begin, uint64_t site_end,
                                      int identity_kind, double *out_host) {
    int rc = check_pairwise_args(ctx, m, site_begin, site_end, "impop_pairwise_identity");
    if (rc) return rc;
    REQUIRE(out_host, "impop_pairwise_identity: out is NULL");
    REQUIRE(identity_kind == IMPOP_IDENTITY_MATCH || identity_kind == IMPOP_IDENTITY_DICE,
            "impop_pairwise_identity: unknown identity kind %d", identity_kind);
    HIP_TRY(hipSetDevice(ctx->device));
    const uint32_t n = m->g.n_hap, ld = m->n_hap_pad;
    Layout L;
    uint64_t *d_W;
    double *d_id;
    L.sub(d_W, 1); L.sub(d_id, (size_t)n * n);
    int32_t *d_g;
    uint32_t *d_add;
    rc = gram_one_window(ctx, m, site_begin, site_end, L, &d_g, &d_add);
    if (rc) return rc;
    const uint64_t W = window_W(m, site_begin, site_end);  // the window's ORIGINAL length
    HIP_TRY(hipMemcpyAsync(d_W, &W, 8, hipMemcpyHostToDevice, ctx->stream));
    SimBatch b{};
    b.gram = d_g; b.stride = (uint64_t)ld * ld; b.ld = ld; b.n = n; b.W = d_W; b.kind = identity_kind; b.round_digits = -1;
    b.add = d_add;
    hipLaunchKernelGGL(identity_dense_kernel, dim3((n + 15) / 16, (n + 15) / 16), dim3(16, 16), 0, ctx->stream, b, n, d_id);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out_host, d_id, (size_t)n * n * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return IMPOP_OK;
}
