// pairwise.hip — the all-pairs path: I_ij = sum_s b_is b_js for every haplotype pair of a
// window, then the full pica2 / h-fst semantics (thresholds, rounding,
// greedy grouping) on identities formed on the fly from the integer Gram matrix.
//
// This path is MFMA-bound, not HBM-bound.  Gram kernel: gram_fp4_kernel (FP4 bit planes, below).
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
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

struct GramWindow {
    uint64_t site_begin, site_end;
};

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
static int launch_gram_unflip(impop_ctx *ctx, const impop_matrix *m, int32_t *d_g, uint64_t n_mats, bool g16 = false) {
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

struct PairFinalIn {
    const Pica2Out *pica;
    const HfstOut *hfst;
    const impop_window_stats *scan;  // integer S / W from the site scan of the same windows
};
__global__ void pairwise_finalize_kernel(PairFinalIn in, uint64_t n_windows, uint32_t nP, int d_pi_mode, int s_scope,
                                         const double *__restrict__ taj /* a1,a2,b1,b2,c1,c2,e1,e2 for n = nP */,
                                         impop_pairwise_stats *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_windows) return;
    const Pica2Out p = in.pica[i];
    const HfstOut h = in.hfst[i];
    const impop_window_stats s = in.scan[i];
    impop_pairwise_stats r;
    r.pi = p.pi; r.pi_site = p.pi_site;
    r.fst = h.v[0]; r.pi_a = h.v[1]; r.pi_b = h.v[2]; r.pi_xy = h.v[3]; r.dxy = h.v[4]; r.da = h.v[5];
    r.n_groups = p.n_groups; r.s_all = s.s_all; r.s_p = s.s_p; r.n_sites = s.n_sites; r.reserved = 0;
    const double S = (double)(s_scope == 0 ? s.s_all : s.s_p);
    const double pin = d_pi_mode == 0 ? py_round(p.pi_site, 8) : d_pi_mode == 1 ? p.pi_site : p.pi * (double)s.n_sites;
    double D = __builtin_nan("");
    if (nP >= 2 && pin == pin && pin >= 0) {
        TajConsts c;
        c.a1 = taj[0]; c.a2 = taj[1]; c.b1 = taj[2]; c.b2 = taj[3]; c.c1 = taj[4]; c.c2 = taj[5]; c.e1 = taj[6]; c.e2 = taj[7];
        D = tajima_d_from(c, S, pin, nullptr, nullptr);
    }
    r.tajima_d = D;
    out[i] = r;
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
static int launch_gram_any(impop_ctx *ctx, const impop_matrix *m, const GramWindow *d_wins, const GramWindow *h_wins,
                           uint32_t n_win, int32_t *d_out, uint64_t max_window_sites, bool *out16 = nullptr) {
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

// W of a window: its length, or the sum of its columns' weights
static inline uint64_t window_W(const impop_matrix *m, uint64_t s0, uint64_t s1) {
    return m->wt_prefix.empty() ? s1 - s0 : m->wt_prefix[s1] - m->wt_prefix[s0];
}

// compacted from a weighted matrix: the summed weights of the dropped all-ones sites of [s0, s1) (original coordinates)
static inline uint32_t ones_weight(const impop_matrix *m, uint64_t s0, uint64_t s1) {
    return (uint32_t)(m->ones_wt_prefix[s1] - m->ones_wt_prefix[s0]);  // < 2^31: part of the window's W
}
static inline bool compact_weighted(const impop_matrix *m) { return m->compact && !m->ones_wt_prefix.empty(); }

}  // namespace impop

using namespace impop;

static int check_pairwise_args(impop_ctx *ctx, const impop_matrix *m, uint64_t s0, uint64_t s1, const char *fn) {
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

IMPOP_API int impop_pairwise_counts(impop_ctx *ctx, const impop_matrix *m, uint64_t site_begin, uint64_t site_end,
                                    int32_t *out_host) {
    int rc = check_pairwise_args(ctx, m, site_begin, site_end, "impop_pairwise_counts");
    if (rc) return rc;
    REQUIRE(out_host, "impop_pairwise_counts: out is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    const uint32_t n = m->g.n_hap, ld = m->n_hap_pad;
    void *d = nullptr;
    Carve L;
    const size_t o_w = L.take<GramWindow>(1), o_g = L.take<int32_t>((size_t)ld * ld), o_ow = L.take<GramWindow>(1), o_add = L.take<uint32_t>(1);
    rc = ctx_scratch(ctx, L.total(), &d);
    if (rc) return rc;
    GramWindow *d_w = L.at<GramWindow>(d, o_w), *d_ow = L.at<GramWindow>(d, o_ow);
    int32_t *d_g = L.at<int32_t>(d, o_g);
    uint32_t *d_add = L.at<uint32_t>(d, o_add);
    GramWindow w;
    map_range(m, site_begin, site_end, &w.site_begin, &w.site_end);  // compacted: the kept sites of the range
    HIP_TRY(hipMemcpyAsync(d_w, &w, sizeof w, hipMemcpyHostToDevice, ctx->stream));
    rc = launch_gram_any(ctx, m, d_w, &w, 1, d_g, w.site_end - w.site_begin);
    if (rc) return rc;
    rc = launch_gram_unflip(ctx, m, d_g, 1);  // exported counts / identities: the original polarity
    if (rc) return rc;
    const GramWindow ow{site_begin, site_end};
    const uint32_t add_w = compact_weighted(m) ? ones_weight(m, site_begin, site_end) : 0u;
    if (m->compact) {  // + the dropped sites every haplotype carries (their count, or their summed weights)
        if (compact_weighted(m)) {
            HIP_TRY(hipMemcpyAsync(d_add, &add_w, 4, hipMemcpyHostToDevice, ctx->stream));
        } else {
            HIP_TRY(hipMemcpyAsync(d_ow, &ow, sizeof ow, hipMemcpyHostToDevice, ctx->stream));
            hipLaunchKernelGGL(seg_count_kernel, dim3(1), dim3(256), 0, ctx->stream, m->d_onesmap, d_ow, 1, (impop_window_stats *)nullptr, d_add);
        }
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
    void *d = nullptr;
    Carve L;
    const size_t o_w = L.take<GramWindow>(1), o_W = L.take<uint64_t>(1), o_g = L.take<int32_t>((size_t)ld * ld),
                 o_id = L.take<double>((size_t)n * n), o_ow = L.take<GramWindow>(1), o_add = L.take<uint32_t>(1);
    rc = ctx_scratch(ctx, L.total(), &d);
    if (rc) return rc;
    GramWindow *d_w = L.at<GramWindow>(d, o_w), *d_ow = L.at<GramWindow>(d, o_ow);
    uint64_t *d_W = L.at<uint64_t>(d, o_W);
    int32_t *d_g = L.at<int32_t>(d, o_g);
    double *d_id = L.at<double>(d, o_id);
    uint32_t *d_add = L.at<uint32_t>(d, o_add);
    GramWindow w;
    map_range(m, site_begin, site_end, &w.site_begin, &w.site_end);
    const uint64_t W = window_W(m, site_begin, site_end);  // the window's ORIGINAL length
    HIP_TRY(hipMemcpyAsync(d_w, &w, sizeof w, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_W, &W, 8, hipMemcpyHostToDevice, ctx->stream));
    rc = launch_gram_any(ctx, m, d_w, &w, 1, d_g, w.site_end - w.site_begin);
    if (rc) return rc;
    rc = launch_gram_unflip(ctx, m, d_g, 1);  // exported counts / identities: the original polarity
    if (rc) return rc;
    SimBatch b{};
    b.gram = d_g; b.stride = (uint64_t)ld * ld; b.ld = ld; b.n = n; b.W = d_W; b.kind = identity_kind; b.round_digits = -1;
    const GramWindow ow{site_begin, site_end};
    const uint32_t add_w = compact_weighted(m) ? ones_weight(m, site_begin, site_end) : 0u;
    if (m->compact) {
        if (compact_weighted(m)) {
            HIP_TRY(hipMemcpyAsync(d_add, &add_w, 4, hipMemcpyHostToDevice, ctx->stream));
        } else {
            HIP_TRY(hipMemcpyAsync(d_ow, &ow, sizeof ow, hipMemcpyHostToDevice, ctx->stream));
            hipLaunchKernelGGL(seg_count_kernel, dim3(1), dim3(256), 0, ctx->stream, m->d_onesmap, d_ow, 1, (impop_window_stats *)nullptr, d_add);
            HIP_TRY(hipGetLastError());
        }
        b.add = d_add;
    }
    hipLaunchKernelGGL(identity_dense_kernel, dim3((n + 15) / 16, (n + 15) / 16), dim3(16, 16), 0, ctx->stream, b, n, d_id);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out_host, d_id, (size_t)n * n * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return IMPOP_OK;
}

// ---- the shared front end of the windowed all-pairs calls (impop_pairwise_scan, impop_cluster_scan) -------------------
// windows -> Gram cells (elementary segments where windows overlap) -> chunks that fit the scratch -> per chunk the Gram
// launch (uint16 counts where they fit), the per-window tables and the filled SimBatch.  What a call does with the
// identities — its epilogue kernels, its records — is the PairEpilogue it hands in.
struct PairChunk {
    SimBatch b;               // the chunk's problems: Gram counts, W, segments, the constant of a compacted matrix
    uint64_t cnt;             // windows (= problems) of the chunk
    const uint64_t *ord;      // problem k is window ord[k] of the caller's list
    uint64_t *d_L;            // seq_len per problem
    impop_window_stats *d_s;  // per problem: n_sites, and S / the scan's sums when the call asked for them
    void *h_out;              // page-locked staging for the chunk's results (out_per_window bytes per problem)
};
struct PairEpilogue {
    virtual ~PairEpilogue() {}
    // once, before the first chunk: d_epi = the epilogue's own device region, sized for chunks of up to cap windows
    virtual int prepare(impop_ctx *ctx, void *d_epi, uint64_t cap) = 0;
    // enqueue the chunk's kernels and the copies of its results into c.h_out (the front end then checks the device error
    // word and synchronises)
    virtual int launch(impop_ctx *ctx, const PairChunk &c) = 0;
    virtual void collect(const PairChunk &c) = 0;  // after the synchronisation: c.h_out -> the caller's arrays
};
struct PairFront {
    const char *fn;
    int identity_kind, round_digits;
    const impop_window_stats *scan_host;  // nullable: the streaming scan's records of the same windows
    bool use_segmap;                      // S of every window from the matrix's site bitmap (into d_s)
    size_t epi_fixed, epi_per_window;     // device bytes of the epilogue: per call, per window of a chunk
    size_t out_per_window;                // staged result bytes per window
    uint64_t max_chunk_windows;           // 0 = no limit of the epilogue's own
};
static int pairwise_front(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows, const PairFront &in,
                          PairEpilogue &epi) {
    const uint32_t ld = m->n_hap_pad, n = m->g.n_hap;
    // IMPOP_TRACE=1: host-side phase times of this call on stderr (where a call's time goes when the kernels are short)
    const bool trace = trace_on();
    const auto t_enter = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (trace) fprintf(stderr, "[%s] %-22s +%.1f us\n", in.fn, what,
                           std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_enter).count());
    };
    // ---- Gram cells.  I_ij is additive over disjoint site ranges, so overlapping (sliding) windows share the
    // Gram matrices of the elementary segments between the sorted window boundaries: every site is
    // contracted once however many windows cover it, and a window is the sum of its consecutive segments
    // (formed on the fly by the statistics kernels, SimBatch.seg_*).  Without overlap the cells are the
    // windows themselves.
    // compacted matrix: the contraction runs over the KEPT (variable) sites of each window; the dropped all-ones
    // sites come back as a per-window constant (SimBatch.add), the dropped all-zero sites contribute nothing
    std::vector<impop_window> mw;
    int rc = map_windows_device(ctx, m, windows, n_windows, mw);
    if (rc) return rc;
    lap("map_windows");
    struct Cell { uint64_t b, e; };
    std::vector<Cell> cells;                                // all Gram cells, in site order when segmented
    std::vector<uint32_t> first(n_windows, 0), count(n_windows, 0);
    std::vector<uint64_t> ord(n_windows);
    for (uint64_t i = 0; i < n_windows; ++i) ord[i] = i;
    // the usual window list — a BED tiling: sorted, no two windows overlapping — has nothing to share: its cells are the windows
    // (one O(n) check instead of the sort + searches below, 0.15 ms of host time per 4096 windows while the GPU waits)
    bool segmented = false;  // cells are elementary segments shared by windows (else: cell k is window k)
    bool tiling = n_windows < 0xFFFFFFF0ull;
    for (uint64_t i = 1; i < n_windows && tiling; ++i) tiling = mw[i].site_begin >= mw[i - 1].site_end && mw[i].site_end >= mw[i].site_begin;
    if (tiling) {
        cells.resize(n_windows);
        for (uint64_t i = 0; i < n_windows; ++i) {
            cells[i] = {mw[i].site_begin, mw[i].site_end};
            first[i] = (uint32_t)i;
            count[i] = 1;
        }
    } else {
        std::vector<uint64_t> cuts;
        uint64_t win_sites = 0;
        for (uint64_t i = 0; i < n_windows; ++i)
            if (mw[i].site_end > mw[i].site_begin) {
                cuts.push_back(mw[i].site_begin);
                cuts.push_back(mw[i].site_end);
                win_sites += mw[i].site_end - mw[i].site_begin;
            }
        std::sort(cuts.begin(), cuts.end());
        cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
        auto at = [&](uint64_t s) { return (size_t)(std::lower_bound(cuts.begin(), cuts.end(), s) - cuts.begin()); };
        std::vector<int64_t> cover(cuts.size() + 1, 0);
        for (uint64_t i = 0; i < n_windows; ++i)
            if (mw[i].site_end > mw[i].site_begin) {
                cover[at(mw[i].site_begin)] += 1;
                cover[at(mw[i].site_end)] -= 1;
            }
        std::vector<uint32_t> seg_before(cuts.size() + 1, 0);  // covered intervals left of cut k
        uint64_t seg_sites = 0;
        int64_t depth = 0;
        std::vector<Cell> segs;
        for (size_t k = 0; k + 1 < cuts.size(); ++k) {
            seg_before[k] = (uint32_t)segs.size();
            depth += cover[k];
            if (depth > 0) {
                segs.push_back({cuts[k], cuts[k + 1]});
                seg_sites += cuts[k + 1] - cuts[k];
            }
        }
        if (!cuts.empty()) seg_before[cuts.size() - 1] = (uint32_t)segs.size();
        if (seg_sites * 20 < win_sites * 19 && segs.size() < 0xFFFFFFF0ull) {  // >= 5 % of the contraction is shared
            cells.swap(segs);
            segmented = true;
            for (uint64_t i = 0; i < n_windows; ++i)
                if (mw[i].site_end > mw[i].site_begin) {
                    first[i] = seg_before[at(mw[i].site_begin)];
                    count[i] = seg_before[at(mw[i].site_end)] - first[i];
                }
            std::stable_sort(ord.begin(), ord.end(), [&](uint64_t a, uint64_t b) {
                const bool ea = count[a] == 0, eb = count[b] == 0;  // empty windows last
                return ea != eb ? eb : (!ea && first[a] < first[b]);
            });
        } else {
            REQUIRE(n_windows < 0xFFFFFFF0ull, "%s: too many windows", in.fn);
            cells.resize(n_windows);
            for (uint64_t i = 0; i < n_windows; ++i) {
                cells[i] = {mw[i].site_begin, mw[i].site_end};
                first[i] = (uint32_t)i;
                count[i] = 1;
            }
        }
    }
    // Chunks of consecutive (in `ord`) windows whose cells fit the Gram scratch (<= ~8 GiB of 288): large
    // chunks keep the persistent Gram grid's last, partially filled round of tasks small next to the launch
    lap("cells");
    const size_t gram_bytes = (size_t)ld * ld * 4;
    uint64_t cap = (8ull << 30) / gram_bytes;  // (a chromosome of 50 kb windows — 4854 on chr2 — is one chunk)
    if (cap > 8192) cap = 8192;
    cap = std::min<uint64_t>(cap, std::max<uint64_t>(cells.size(), n_windows));  // a short call stages (and copies) short tables
    if (cap < 1) cap = 1;
    // windows per chunk: the Gram capacity, what the epilogue's own buffers allow, and the test switch IMPOP_PAIRWISE_CHUNK
    // (windows per chunk: forces several chunks on lists far too short to need them; records must not change)
    uint64_t win_cap = cap;
    if (in.max_chunk_windows) win_cap = std::min<uint64_t>(win_cap, std::max<uint64_t>(in.max_chunk_windows, 1));
    static const uint64_t chunk_env = [] { const char *e = getenv("IMPOP_PAIRWISE_CHUNK"); return e ? strtoull(e, nullptr, 10) : 0ull; }();
    if (chunk_env) win_cap = std::min<uint64_t>(win_cap, chunk_env);
    // one cell per window: a chunk never holds more Gram matrices than windows, so the Gram and table scratch is sized for that
    // (an epilogue that allows ~100 windows per chunk would otherwise reserve room for 8192 matrices it can never fill)
    if (!segmented) cap = std::min<uint64_t>(cap, win_cap);
    // per-chunk metadata: ONE contiguous region mirrored on the host, so that a chunk costs one host-to-device copy
    // (eight small pageable copies were ~0.3 ms of host time between two Gram launches)
    Carve M;  // cells first: they go up on their own, everything from o_W on in a second copy
    const size_t o_w = M.take<GramWindow>(cap), o_W = M.take<uint64_t>(cap), o_L = M.take<uint64_t>(cap), o_first = M.take<uint32_t>(cap),
                 o_count = M.take<uint32_t>(cap), o_s = M.take<impop_window_stats>(cap), o_sw = M.take<GramWindow>(cap),
                 o_ow = M.take<GramWindow>(cap), meta_bytes = M.total();
    const size_t epi_bytes = in.epi_fixed + win_cap * in.epi_per_window;
    Carve D;  // device: Gram matrices | metadata | compacted: dropped all-ones sites per window | the epilogue's own region
    const size_t o_g = D.take_bytes(cap * gram_bytes), o_meta = D.take_bytes(meta_bytes), o_add = D.take<uint32_t>(cap),
                 o_epi = D.take_bytes(epi_bytes);
    void *d = nullptr;
    rc = ctx_scratch(ctx, D.total(), &d);
    if (rc) return rc;
    int32_t *d_g = D.at<int32_t>(d, o_g);
    char *d_meta = D.at<char>(d, o_meta);
    GramWindow *d_w = M.at<GramWindow>(d_meta, o_w);
    uint64_t *d_W = M.at<uint64_t>(d_meta, o_W), *d_L = M.at<uint64_t>(d_meta, o_L);
    uint32_t *d_first = M.at<uint32_t>(d_meta, o_first), *d_count = M.at<uint32_t>(d_meta, o_count);
    impop_window_stats *d_s = M.at<impop_window_stats>(d_meta, o_s);
    GramWindow *d_sw = M.at<GramWindow>(d_meta, o_sw);  // the chunk's WINDOWS (d_w holds its Gram cells), matrix coordinates
    GramWindow *d_ow = M.at<GramWindow>(d_meta, o_ow);  // the same windows in ORIGINAL coordinates (compacted matrices)
    uint32_t *d_add = D.at<uint32_t>(d, o_add);
    void *d_epi = D.at<char>(d, o_epi);
    rc = epi.prepare(ctx, d_epi, win_cap);
    if (rc) return rc;
    // even out the chunks: a total slightly above the capacity would otherwise leave a last chunk of a few
    // windows whose single-workgroup epilogue kernels cost their full latency
    uint64_t cell_limit = cap;
    if (cells.size() > cap) {
        uint32_t widest = 1;
        for (uint64_t i = 0; i < n_windows; ++i) widest = std::max(widest, count[i]);
        uint64_t n_chunks = (cells.size() + cap - 1) / cap;
        if ((cells.size() + n_chunks - 1) / n_chunks + widest > cap) ++n_chunks;  // neighbours re-contract up to `widest` cells
        cell_limit = std::min<uint64_t>(cap, (cells.size() + n_chunks - 1) / n_chunks + widest);
    }
    lap("scratch");
    // page-locked staging for the metadata going up and the results coming down (ctx_pinned)
    const size_t out_off = meta_bytes;
    void *pin = nullptr;
    rc = ctx_pinned(ctx, out_off + win_cap * in.out_per_window, &pin);
    if (rc) return rc;
    char *hmeta = reinterpret_cast<char *>(pin);
    memset(hmeta, 0, meta_bytes);
    GramWindow *gw = M.at<GramWindow>(hmeta, o_w), *swv = M.at<GramWindow>(hmeta, o_sw), *owv = M.at<GramWindow>(hmeta, o_ow);
    uint64_t *Wv = M.at<uint64_t>(hmeta, o_W), *Lv = M.at<uint64_t>(hmeta, o_L);
    uint32_t *fv = M.at<uint32_t>(hmeta, o_first), *cvv = M.at<uint32_t>(hmeta, o_count);
    impop_window_stats *sv = M.at<impop_window_stats>(hmeta, o_s);
    std::vector<uint32_t> add_h;
    uint64_t call_max_W = 0;  // bounds every Gram count of the call (a cell is a window or a piece of one; compacted: + its constant)
    for (uint64_t i = 0; i < n_windows; ++i) call_max_W = std::max(call_max_W, window_W(m, windows[i].site_begin, windows[i].site_end));
    bool g16 = false;
    for (uint64_t base = 0; base < n_windows;) {
        // windows ord[base .. base+cnt): their cells are [c_lo, c_hi)
        uint64_t cnt = 0;
        uint32_t c_lo = 0, c_hi = 0;
        bool have = false;
        while (base + cnt < n_windows && cnt < cell_limit && cnt < win_cap) {
            const uint64_t wdx = ord[base + cnt];
            if (count[wdx]) {
                const uint32_t lo = have ? std::min(c_lo, first[wdx]) : first[wdx];
                const uint32_t hi = have ? std::max(c_hi, first[wdx] + count[wdx]) : first[wdx] + count[wdx];
                if ((uint64_t)(hi - lo) > (cnt == 0 ? cap : cell_limit)) {
                    REQUIRE(cnt != 0, "%s: window %llu spans %u segments, more than the %llu Gram matrices that fit the scratch", in.fn,
                            (unsigned long long)wdx, count[wdx], (unsigned long long)cap);
                    break;
                }
                c_lo = lo; c_hi = hi; have = true;
            }
            ++cnt;
        }
        const uint32_t n_cells = have ? c_hi - c_lo : 0;
        uint64_t max_sites = 0;
        for (uint32_t c = 0; c < n_cells; ++c) {
            gw[c] = {cells[c_lo + c].b, cells[c_lo + c].e};
            max_sites = std::max<uint64_t>(max_sites, cells[c_lo + c].e - cells[c_lo + c].b);
        }
        // the Gram launch needs the cells alone: they go up first and the kernel starts, the per-window tables are filled in (and
        // copied) while it runs
        if (n_cells) HIP_TRY(hipMemcpyAsync(d_meta + o_w, hmeta + o_w, (size_t)n_cells * sizeof(GramWindow), hipMemcpyHostToDevice, ctx->stream));
        if (n_cells) {
            size_t slot = 0;  // impop_ctx_gram_timing: the Gram launch(es) of this chunk between two events
            if (ctx->gram_timing && (rc = ctx->gram_timer.begin(ctx->stream, &slot))) return rc;
            // counts as uint16 where every count of the call fits (a count is at most its window's W): half the result bytes
            static const bool u16_off = env_is("IMPOP_GRAM_U16", '0');
            g16 = !u16_off && call_max_W < 65536;
            rc = launch_gram_any(ctx, m, d_w, gw, n_cells, d_g, max_sites, &g16);
            if (rc) return rc;
            if (ctx->gram_timing && (rc = ctx->gram_timer.end(ctx->stream, slot))) return rc;
            if (in.identity_kind != IMPOP_IDENTITY_MATCH) {  // `match` sees Hamming distances only: polarity-invariant
                rc = launch_gram_unflip(ctx, m, d_g, n_cells, g16);
                if (rc) return rc;
            }
        }
        for (uint64_t k = 0; k < cnt; ++k) {
            const uint64_t wdx = ord[base + k];
            Wv[k] = window_W(m, windows[wdx].site_begin, windows[wdx].site_end);
            Lv[k] = windows[wdx].seq_len;
            fv[k] = count[wdx] ? first[wdx] - c_lo : 0;
            cvv[k] = count[wdx];
            if (in.scan_host) sv[k] = in.scan_host[wdx];
            else { memset(&sv[k], 0, sizeof(sv[k])); sv[k].n_sites = (uint32_t)Wv[k]; }
            swv[k] = {mw[wdx].site_begin, mw[wdx].site_end};
            owv[k] = {windows[wdx].site_begin, windows[wdx].site_end};
        }
        // problem k IS Gram matrix k (disjoint windows, none empty): the epilogue kernels then take their one-matrix variants
        bool one_to_one = true;
        for (uint64_t k = 0; k < cnt && one_to_one; ++k) one_to_one = cvv[k] == 1 && fv[k] == k;
        lap("chunk metadata");
        HIP_TRY(hipMemcpyAsync(d_meta + o_W, hmeta + o_W, meta_bytes - o_W, hipMemcpyHostToDevice, ctx->stream));
        if (in.use_segmap) {
            hipLaunchKernelGGL(seg_count_kernel, dim3((uint32_t)((cnt + 3) / 4)), dim3(256), 0, ctx->stream, m->d_segmap, d_sw, cnt, d_s,
                               (uint32_t *)nullptr);
            HIP_TRY(hipGetLastError());
        }
        PairChunk ch{};
        SimBatch &b = ch.b;
        b.gram = d_g; b.stride = (uint64_t)ld * ld; b.ld = ld; b.n = n; b.W = d_W; b.kind = in.identity_kind;
        b.g16 = g16 ? 1u : 0u;
        b.max_W = call_max_W;
        b.round_digits = in.round_digits < 0 ? -1 : in.round_digits;
        b.seg_first = one_to_one ? nullptr : d_first; b.seg_count = one_to_one ? nullptr : d_count;
        if (compact_weighted(m)) {  // the dropped all-ones sites' summed weights, from the host prefix sums
            add_h.resize(cnt);
            for (uint64_t k = 0; k < cnt; ++k) add_h[k] = ones_weight(m, windows[ord[base + k]].site_begin, windows[ord[base + k]].site_end);
            HIP_TRY(hipMemcpyAsync(d_add, add_h.data(), cnt * 4, hipMemcpyHostToDevice, ctx->stream));
            b.add = d_add;
        } else if (m->compact) {    // ... their count, from the bitmap on the device
            hipLaunchKernelGGL(seg_count_kernel, dim3((uint32_t)((cnt + 3) / 4)), dim3(256), 0, ctx->stream, m->d_onesmap, d_ow, cnt,
                               (impop_window_stats *)nullptr, d_add);
            HIP_TRY(hipGetLastError());
            b.add = d_add;
        }
        ch.cnt = cnt; ch.ord = ord.data() + base; ch.d_L = d_L; ch.d_s = d_s; ch.h_out = hmeta + out_off;
        rc = epi.launch(ctx, ch);
        if (rc) return rc;
        lap("chunk launched");
        rc = ctx_err_fetch(ctx);
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(ctx->stream));  // the staging vectors are reused by the next chunk
        rc = ctx_err_result(ctx, in.fn);  // a device-side consistency check tripped: no partial results
        if (rc) return rc;
        epi.collect(ch);
        base += cnt;
        lap("chunk done");
    }
    return IMPOP_OK;
}

namespace {
// impop_pairwise_scan's epilogue: pica2 grouping next to the Fst sums, then the fixed records
struct PairwiseStatsEpilogue final : PairEpilogue {
    const impop_pairwise_params *params;
    const uint64_t *mask_p;
    uint32_t n, nP;
    bool want_s;
    const std::vector<uint32_t> *idx, *ia, *ib;
    const std::vector<uint8_t> *fa, *fb;
    impop_pairwise_stats *out_host;
    Pica2Out *d_p = nullptr;
    HfstOut *d_h = nullptr;
    impop_pairwise_stats *d_o = nullptr;
    uint32_t *d_idx = nullptr, *d_ia = nullptr, *d_ib = nullptr;
    uint8_t *d_fa = nullptr, *d_fb = nullptr;
    // prepare()'s member lists and flags; + 256: the total of its layout is rounded up
    static size_t fixed_bytes(uint32_t n) { return 3 * round_up_256((size_t)(n ? n : 1) * 4) + 2 * round_up_256(n ? n : 1) + 256; }
    static size_t window_bytes() { return sizeof(Pica2Out) + sizeof(HfstOut) + sizeof(impop_pairwise_stats); }
    int prepare(impop_ctx *ctx, void *d_epi, uint64_t cap) override {
        Carve L;
        d_idx = L.at<uint32_t>(d_epi, L.take<uint32_t>(n ? n : 1));
        d_ia = L.at<uint32_t>(d_epi, L.take<uint32_t>(n ? n : 1));
        d_ib = L.at<uint32_t>(d_epi, L.take<uint32_t>(n ? n : 1));
        d_fa = L.at<uint8_t>(d_epi, L.take<uint8_t>(n ? n : 1));
        d_fb = L.at<uint8_t>(d_epi, L.take<uint8_t>(n ? n : 1));
        char *w = L.at<char>(d_epi, L.take_bytes(cap * window_bytes()));
        d_h = reinterpret_cast<HfstOut *>(w);
        d_o = reinterpret_cast<impop_pairwise_stats *>(w + cap * sizeof(HfstOut));
        d_p = reinterpret_cast<Pica2Out *>(w + cap * (sizeof(HfstOut) + sizeof(impop_pairwise_stats)));
        if (nP) HIP_TRY(hipMemcpyAsync(d_idx, idx->data(), (size_t)nP * 4, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(d_fa, fa->data(), n, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(d_fb, fb->data(), n, hipMemcpyHostToDevice, ctx->stream));
        if (!ia->empty()) HIP_TRY(hipMemcpyAsync(d_ia, ia->data(), ia->size() * 4, hipMemcpyHostToDevice, ctx->stream));
        if (!ib->empty()) HIP_TRY(hipMemcpyAsync(d_ib, ib->data(), ib->size() * 4, hipMemcpyHostToDevice, ctx->stream));
        return IMPOP_OK;
    }
    int launch(impop_ctx *ctx, const PairChunk &c) override {
        const SimBatch &b = c.b;
        const uint64_t cnt = c.cnt;
        // pica2 grouping and the Fst sums are independent, latency-bound one-workgroup-per-window kernels: pica2 goes
        // to the side stream (fork behind the Gram launch, join before the finalize) so the two overlap
        if (!ctx->side) {
            HIP_TRY(hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming));
        }
        HIP_TRY(hipEventRecord(ctx->ev_fork, ctx->stream));
        HIP_TRY(hipStreamWaitEvent(ctx->side, ctx->ev_fork, 0));
        hipStream_t main_stream = ctx->stream;
        ctx->stream = ctx->side;
        int rc = launch_pica2(ctx, b, cnt, mask_p ? d_idx : nullptr, nP, nullptr, params->threshold, c.d_L, d_p, nullptr);
        ctx->stream = main_stream;
        if (rc) return rc;
        HIP_TRY(hipEventRecord(ctx->ev_join, ctx->side));
        if (params->fst_method == 1)
            rc = launch_hud_grouped(ctx, b, cnt, d_ia, (uint32_t)ia->size(), d_ib, (uint32_t)ib->size(), nullptr, nullptr, params->threshold,
                                    c.d_L, d_h);
        else
            rc = launch_hfst(ctx, b, cnt, d_fa, d_fb, c.d_L, d_h);
        if (rc) return rc;
        HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
        PairFinalIn in{d_p, d_h, c.d_s};
        rc = ensure_tajima_consts(ctx, nP >= 2 ? (int64_t)nP : 2);  // the cache may have been retargeted by another plan
        if (rc) return rc;
        hipLaunchKernelGGL(pairwise_finalize_kernel, dim3((uint32_t)((cnt + 63) / 64)), dim3(64), 0, ctx->stream, in, cnt,
                           want_s ? nP : 0u, params->d_pi_mode, want_s ? params->s_scope : 0, ctx->d_taj, d_o);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(c.h_out, d_o, cnt * sizeof(impop_pairwise_stats), hipMemcpyDeviceToHost, ctx->stream));
        return IMPOP_OK;
    }
    void collect(const PairChunk &c) override {
        const impop_pairwise_stats *ov = reinterpret_cast<const impop_pairwise_stats *>(c.h_out);
        for (uint64_t k = 0; k < c.cnt; ++k) out_host[c.ord[k]] = ov[k];
    }
};

// impop_cluster_scan's epilogue: one clustering launch (stats_kernels.h launch_af_batch), records and member tables
struct ClusterEpilogue final : PairEpilogue {
    const impop_cluster_params *params;
    const uint64_t *mask_p;
    uint32_t nP;
    const std::vector<uint32_t> *idx;
    impop_cluster_stats *out_host;
    uint32_t *cluster_of, *sizes;
    size_t adj_bytes = 0;  // per window: the general form's adjacency rows (0 when the call is sure to take the window-shape kernel)
    impop_cluster_stats *d_rec = nullptr;
    uint32_t *d_idx = nullptr, *d_cl = nullptr, *d_sz = nullptr, *d_adj = nullptr;
    size_t members_bytes() const { return (size_t)nP * 4; }
    bool want_members() const { return cluster_of || sizes; }
    static size_t fixed_bytes(uint32_t nP) { return round_up_256((size_t)(nP ? nP : 1) * 4) + 4 * 256; }
    // the window-shape kernel writes tables only when asked; the general form always writes both (sizes is its ranking's output)
    size_t tables_bytes() const { return (adj_bytes == 0 && !want_members()) ? 0 : 2 * members_bytes(); }
    size_t window_bytes() const { return sizeof(impop_cluster_stats) + tables_bytes() + adj_bytes; }
    int prepare(impop_ctx *ctx, void *d_epi, uint64_t cap) override {
        Carve L;
        d_idx = L.at<uint32_t>(d_epi, L.take<uint32_t>(nP ? nP : 1));
        d_rec = L.at<impop_cluster_stats>(d_epi, L.take<impop_cluster_stats>(cap));
        // (the layout's alignment gaps and rounded total: fixed_bytes' 4 x 256)
        char *w = L.at<char>(d_epi, L.take_bytes(cap * (tables_bytes() + adj_bytes)));
        d_cl = reinterpret_cast<uint32_t *>(w);
        d_sz = reinterpret_cast<uint32_t *>(w + cap * (tables_bytes() / 2));
        d_adj = reinterpret_cast<uint32_t *>(w + cap * tables_bytes());
        if (nP) HIP_TRY(hipMemcpyAsync(d_idx, idx->data(), (size_t)nP * 4, hipMemcpyHostToDevice, ctx->stream));
        return IMPOP_OK;
    }
    // staged per chunk: cnt records | cnt x nP cluster_of | cnt x nP sizes (the tables only when asked for)
    int launch(impop_ctx *ctx, const PairChunk &c) override {
        const uint64_t cnt = c.cnt;
        size_t slot = 0;  // the clustering kernel(s) between two events of their own: impop_ctx_cluster_elapsed
        int rc = ctx->gram_timing ? ctx->cluster_timer.begin(ctx->stream, &slot) : IMPOP_OK;
        if (rc) return rc;
        rc = launch_af_batch(ctx, c.b, cnt, mask_p ? d_idx : nullptr, nP, params->threshold, d_adj, adj_bytes, d_rec, d_cl, d_sz, want_members());
        if (rc) return rc;
        if (ctx->gram_timing && (rc = ctx->cluster_timer.end(ctx->stream, slot))) return rc;
        char *h = reinterpret_cast<char *>(c.h_out);
        HIP_TRY(hipMemcpyAsync(h, d_rec, cnt * sizeof(impop_cluster_stats), hipMemcpyDeviceToHost, ctx->stream));
        if (want_members() && nP) {
            h += cnt * sizeof(impop_cluster_stats);
            if (cluster_of) HIP_TRY(hipMemcpyAsync(h, d_cl, cnt * members_bytes(), hipMemcpyDeviceToHost, ctx->stream));
            if (sizes) HIP_TRY(hipMemcpyAsync(h + cnt * members_bytes(), d_sz, cnt * members_bytes(), hipMemcpyDeviceToHost, ctx->stream));
        }
        return IMPOP_OK;
    }
    void collect(const PairChunk &c) override {
        const char *h = reinterpret_cast<const char *>(c.h_out);
        const impop_cluster_stats *rv = reinterpret_cast<const impop_cluster_stats *>(h);
        const char *hc = h + c.cnt * sizeof(impop_cluster_stats), *hs = hc + c.cnt * members_bytes();
        for (uint64_t k = 0; k < c.cnt; ++k) {
            out_host[c.ord[k]] = rv[k];
            if (cluster_of && nP) memcpy(cluster_of + c.ord[k] * nP, hc + k * members_bytes(), members_bytes());
            if (sizes && nP) memcpy(sizes + c.ord[k] * nP, hs + k * members_bytes(), members_bytes());
        }
    }
};
// impop_pairwise_scan_panel's records from the per-panel pica2 results, the per-pair Fst results and the window's S / W: one thread
// per (window, panel or pair); the arithmetic of a panel record is pairwise_finalize_kernel's with nP = the panel's size
struct PanelFinalIn {
    const Pica2Out *pica;            // panel k of problem w at k * stride + w
    const HfstOut *hfst;             // pair p of problem w at p * stride + w; nullptr: no pair records asked for
    const impop_window_stats *scan;  // n_sites, and s_all from the site bitmap (s_scope 0, 1)
    const uint32_t *s_p;             // s_scope 1: panel k of problem w at k * stride + w
    const double *taj;               // a1,a2,b1,b2,c1,c2,e1,e2 per panel
    const uint32_t *n_members;       // per panel
    uint64_t stride;
};
__global__ void panel_finalize_kernel(PanelFinalIn in, uint64_t n_windows, uint32_t K, int d_pi_mode, int s_scope,
                                      impop_panel_stats *__restrict__ out_panels, impop_pair_stats *__restrict__ out_pairs,
                                      impop_panel_window *__restrict__ out_windows) {
    const uint32_t NP = in.hfst ? K * (K - 1) / 2 : 0u, items = K + NP;
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_windows * items) return;
    const uint64_t w = t / items;
    const uint32_t j = (uint32_t)(t % items);
    if (j >= K) {
        const HfstOut h = in.hfst[(uint64_t)(j - K) * in.stride + w];
        impop_pair_stats r;
        r.fst = h.v[0]; r.pi_a = h.v[1]; r.pi_b = h.v[2]; r.pi_xy = h.v[3]; r.dxy = h.v[4]; r.da = h.v[5];
        out_pairs[w * NP + (j - K)] = r;
        return;
    }
    const impop_window_stats s = in.scan[w];
    if (j == 0) out_windows[w] = impop_panel_window{s.n_sites, s.s_all};
    const Pica2Out p = in.pica[(uint64_t)j * in.stride + w];
    const uint32_t nP = in.n_members[j], sp = s_scope == 1 ? in.s_p[(uint64_t)j * in.stride + w] : 0u;
    impop_panel_stats r;
    r.pi = p.pi; r.pi_site = p.pi_site;
    r.n_members = nP; r.n_groups = p.n_groups; r.s_p = sp; r.reserved = 0; r.reserved2 = 0;
    const double S = (double)(s_scope == 1 ? sp : s.s_all);
    const double pin = d_pi_mode == 0 ? py_round(p.pi_site, 8) : d_pi_mode == 1 ? p.pi_site : p.pi * (double)s.n_sites;
    double D = __builtin_nan("");
    if (s_scope != 2 && nP >= 2 && pin == pin && pin >= 0) {
        const double *tj = in.taj + 8 * j;
        TajConsts c;
        c.a1 = tj[0]; c.a2 = tj[1]; c.b1 = tj[2]; c.b2 = tj[3]; c.c1 = tj[4]; c.c2 = tj[5]; c.e1 = tj[6]; c.e2 = tj[7];
        D = tajima_d_from(c, S, pin, nullptr, nullptr);
    }
    r.tajima_d = D;
    out_panels[w * K + j] = r;
}

// impop_pairwise_scan_panel's epilogue: K panels and their K (K - 1) / 2 pairs on the chunk's ONE set of Gram matrices — pica2 per
// panel on the side stream, next to it the Fst sums of all pairs (one launch of hfst_panel_small_kernel on the window-statistics
// shape; launch_hfst per pair on every other), then the records
struct PanelEpilogue final : PairEpilogue {
    const impop_pairwise_params *params;
    uint32_t n, K, NP;                      // NP = 0: no pair records asked for
    const std::vector<uint32_t> *idx;       // the panels' members back to back, each ascending
    const std::vector<uint32_t> *sizes;     // members per panel
    const std::vector<uint8_t> *cls;        // class of haplotype i, 0xFF: none
    const std::vector<uint32_t> *sp_host;   // s_scope 1: K x n_windows, panel-major; else nullptr
    uint64_t n_windows;
    impop_panel_stats *out_panels;
    impop_pair_stats *out_pairs;
    impop_panel_window *out_windows;
    bool traced = false;
    uint64_t cap = 0;
    Pica2Out *d_p = nullptr;
    HfstOut *d_h = nullptr;
    impop_panel_stats *d_opan = nullptr;
    impop_pair_stats *d_opair = nullptr;
    impop_panel_window *d_owin = nullptr;
    uint32_t *d_idx = nullptr, *d_sizes = nullptr, *d_sp = nullptr;
    uint8_t *d_cls = nullptr, *d_flags = nullptr;  // d_flags: K x n membership flags (the general route's in_a / in_b)
    double *d_taj = nullptr;
    std::vector<uint32_t> sp_chunk;
    // the member list, sizes, Tajima constants, classes and flags, plus the layout's alignment gaps (fifteen sub-buffers)
    static size_t fixed_bytes(uint32_t n, uint32_t K) {
        return round_up_256((size_t)(n ? n : 1) * 4) + 2 * round_up_256((size_t)K * 8 * 8) + round_up_256(n ? n : 1) +
               round_up_256((size_t)K * (n ? n : 1)) + 16 * 256;
    }
    static size_t window_bytes(uint32_t K, uint32_t NP) {
        return (size_t)K * (sizeof(Pica2Out) + sizeof(impop_panel_stats) + 4) + (size_t)NP * (sizeof(HfstOut) + sizeof(impop_pair_stats)) +
               sizeof(impop_panel_window);
    }
    static size_t staged_bytes(uint32_t K, uint32_t NP) {
        return (size_t)K * sizeof(impop_panel_stats) + (size_t)NP * sizeof(impop_pair_stats) + sizeof(impop_panel_window);
    }
    int prepare(impop_ctx *ctx, void *d_epi, uint64_t cap_) override {
        cap = cap_;
        Carve L;
        d_idx = L.at<uint32_t>(d_epi, L.take<uint32_t>(n ? n : 1));
        d_sizes = L.at<uint32_t>(d_epi, L.take<uint32_t>(K));
        d_taj = L.at<double>(d_epi, L.take<double>((size_t)K * 8));
        d_cls = L.at<uint8_t>(d_epi, L.take<uint8_t>(n ? n : 1));
        d_flags = L.at<uint8_t>(d_epi, L.take<uint8_t>((size_t)K * (n ? n : 1)));
        d_p = L.at<Pica2Out>(d_epi, L.take<Pica2Out>(cap * K));
        d_h = L.at<HfstOut>(d_epi, L.take<HfstOut>(cap * NP));
        d_opan = L.at<impop_panel_stats>(d_epi, L.take<impop_panel_stats>(cap * K));
        d_opair = L.at<impop_pair_stats>(d_epi, L.take<impop_pair_stats>(cap * NP));
        d_owin = L.at<impop_panel_window>(d_epi, L.take<impop_panel_window>(cap));
        d_sp = L.at<uint32_t>(d_epi, L.take<uint32_t>(cap * K));
        if (!idx->empty()) HIP_TRY(hipMemcpyAsync(d_idx, idx->data(), idx->size() * 4, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(d_sizes, sizes->data(), (size_t)K * 4, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(d_cls, cls->data(), n, hipMemcpyHostToDevice, ctx->stream));
        flags_host.assign((size_t)K * n, 0);
        for (uint32_t i = 0; i < n; ++i)
            if ((*cls)[i] < K) flags_host[(size_t)(*cls)[i] * n + i] = 1;
        HIP_TRY(hipMemcpyAsync(d_flags, flags_host.data(), flags_host.size(), hipMemcpyHostToDevice, ctx->stream));
        for (uint32_t k = 0; k < K; ++k) {  // the context caches the constants of ONE n: each panel's are copied out behind their kernel
            const int rc = ensure_tajima_consts(ctx, (*sizes)[k] >= 2 ? (int64_t)(*sizes)[k] : 2);
            if (rc) return rc;
            HIP_TRY(hipMemcpyAsync(d_taj + 8 * k, ctx->d_taj, 8 * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        }
        return IMPOP_OK;
    }
    std::vector<uint8_t> flags_host;
    int launch(impop_ctx *ctx, const PairChunk &c) override {
        const SimBatch &b = c.b;
        const uint64_t cnt = c.cnt;
        const bool small = hfst_panel_small_applies(b);
        if (!traced && trace_on())
            fprintf(stderr, "[impop_pairwise_scan_panel] pops=%u pairs=%u route=%s\n", K, K * (K - 1) / 2, small ? "small" : "general");
        traced = true;
        if (!ctx->side) {
            HIP_TRY(hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming));
        }
        if (sp_host) {  // s_scope 1: the chunk's rows of the streaming scan's s_p, in the chunk's problem order
            sp_chunk.resize((size_t)K * cap);
            for (uint32_t k = 0; k < K; ++k)
                for (uint64_t i = 0; i < cnt; ++i) sp_chunk[(size_t)k * cap + i] = (*sp_host)[(size_t)k * n_windows + c.ord[i]];
            HIP_TRY(hipMemcpyAsync(d_sp, sp_chunk.data(), (size_t)K * cap * 4, hipMemcpyHostToDevice, ctx->stream));
        }
        HIP_TRY(hipEventRecord(ctx->ev_fork, ctx->stream));
        HIP_TRY(hipStreamWaitEvent(ctx->side, ctx->ev_fork, 0));
        hipStream_t main_stream = ctx->stream;
        ctx->stream = ctx->side;
        int rc = IMPOP_OK;
        for (uint32_t k = 0, at = 0; k < K && !rc; at += (*sizes)[k], ++k)
            rc = launch_pica2(ctx, b, cnt, d_idx + at, (*sizes)[k], nullptr, params->threshold, c.d_L, d_p + (uint64_t)k * cap, nullptr);
        ctx->stream = main_stream;
        if (rc) return rc;
        HIP_TRY(hipEventRecord(ctx->ev_join, ctx->side));
        if (NP) {
            size_t slot = 0;  // impop_ctx_gram_timing: the Fst kernel(s) of the chunk between two events (impop_ctx_cluster_elapsed)
            if (ctx->gram_timing && (rc = ctx->cluster_timer.begin(ctx->stream, &slot))) return rc;
            if (small) {
                rc = launch_hfst_panel_small(ctx, b, cnt, d_cls, K, c.d_L, d_h, cap);
            } else {
                uint32_t p = 0;
                for (uint32_t a = 0; a < K && !rc; ++a)
                    for (uint32_t bb = a + 1; bb < K && !rc; ++bb, ++p)
                        rc = launch_hfst(ctx, b, cnt, d_flags + (size_t)a * n, d_flags + (size_t)bb * n, c.d_L, d_h + (uint64_t)p * cap);
            }
            if (rc) return rc;
            if (ctx->gram_timing && (rc = ctx->cluster_timer.end(ctx->stream, slot))) return rc;
        }
        HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
        PanelFinalIn in{d_p, NP ? d_h : nullptr, c.d_s, sp_host ? d_sp : nullptr, d_taj, d_sizes, cap};
        const uint64_t items = cnt * (K + NP);
        hipLaunchKernelGGL(panel_finalize_kernel, dim3((uint32_t)((items + 127) / 128)), dim3(128), 0, ctx->stream, in, cnt, K,
                           params->d_pi_mode, params->s_scope, d_opan, d_opair, d_owin);
        HIP_TRY(hipGetLastError());
        char *h = reinterpret_cast<char *>(c.h_out);
        HIP_TRY(hipMemcpyAsync(h, d_opan, cnt * K * sizeof(impop_panel_stats), hipMemcpyDeviceToHost, ctx->stream));
        h += cnt * K * sizeof(impop_panel_stats);
        if (NP) HIP_TRY(hipMemcpyAsync(h, d_opair, cnt * NP * sizeof(impop_pair_stats), hipMemcpyDeviceToHost, ctx->stream));
        h += cnt * NP * sizeof(impop_pair_stats);
        HIP_TRY(hipMemcpyAsync(h, d_owin, cnt * sizeof(impop_panel_window), hipMemcpyDeviceToHost, ctx->stream));
        return IMPOP_OK;
    }
    void collect(const PairChunk &c) override {
        const char *h = reinterpret_cast<const char *>(c.h_out);
        const impop_panel_stats *pv = reinterpret_cast<const impop_panel_stats *>(h);
        const impop_pair_stats *qv = reinterpret_cast<const impop_pair_stats *>(h + c.cnt * K * sizeof(impop_panel_stats));
        const impop_panel_window *wv =
            reinterpret_cast<const impop_panel_window *>(h + c.cnt * (K * sizeof(impop_panel_stats) + NP * sizeof(impop_pair_stats)));
        for (uint64_t k = 0; k < c.cnt; ++k) {
            memcpy(out_panels + c.ord[k] * K, pv + k * K, (size_t)K * sizeof(impop_panel_stats));
            if (NP) memcpy(out_pairs + c.ord[k] * NP, qv + k * NP, (size_t)NP * sizeof(impop_pair_stats));
            if (out_windows) out_windows[c.ord[k]] = wv[k];
        }
    }
};
}  // namespace
static_assert(sizeof(impop_panel_stats) == 48 && sizeof(impop_panel_window) == 8 && sizeof(impop_pair_stats) == 48, "fixed record layouts");

IMPOP_API int impop_pairwise_scan_panel(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows,
                                        const uint64_t *masks, uint32_t n_pop, const impop_pairwise_params *params,
                                        impop_panel_stats *out_panels, impop_pair_stats *out_pairs, impop_panel_window *out_windows) {
    const char *fn = "impop_pairwise_scan_panel";
    REQUIRE(ctx && m && params, "%s: NULL argument", fn);
    REQUIRE(params->struct_size == sizeof(impop_pairwise_params), "impop_pairwise_params.struct_size mismatch");
    REQUIRE(params->identity_kind == IMPOP_IDENTITY_MATCH || params->identity_kind == IMPOP_IDENTITY_DICE, "%s: unknown identity kind", fn);
    REQUIRE(params->round_digits <= 19, "%s: round_digits > 19 unsupported", fn);
    REQUIRE(params->d_pi_mode >= 0 && params->d_pi_mode <= 2 && params->s_scope >= 0 && params->s_scope <= 2, "%s: bad d_pi_mode / s_scope", fn);
    REQUIRE(params->fst_method <= 1, "%s: fst_method must be 0 (direct)", fn);
    if (params->fst_method == 1) {
        set_error("%s: fst_method 1 (hud.py grouped) is not available for panels; use impop_pairwise_scan per pair", fn);
        return IMPOP_E_UNSUPPORTED;
    }
    REQUIRE(n_pop >= 2 && n_pop <= 8, "%s: n_pop must be 2..8", fn);
    REQUIRE(masks, "%s: masks is NULL", fn);
    const uint32_t n = m->g.n_hap, K = n_pop, mwords = (n + 63) / 64;
    std::vector<uint8_t> cls(n, 0xFF);
    std::vector<uint32_t> idx, sizes(K, 0);
    for (uint32_t k = 0; k < K; ++k) {
        const uint64_t *mk = masks + (size_t)k * mwords;
        for (uint32_t i = 0; i < n; ++i) {
            if (!((mk[i >> 6] >> (i & 63)) & 1ull)) continue;
            // h-fst.py:181-185 removes shared members per pair, which would make a panel's size depend on the pair
            REQUIRE(cls[i] == 0xFF, "%s: populations must be disjoint (population %u overlaps population %u)", fn, k, (uint32_t)cls[i]);
            cls[i] = (uint8_t)k;
            idx.push_back(i);
            ++sizes[k];
        }
        REQUIRE(sizes[k] > 0, "%s: population %u is empty", fn, k);
    }
    if (!n_windows) return IMPOP_OK;
    REQUIRE(windows && out_panels, "%s: NULL windows/out", fn);
    for (uint64_t i = 0; i < n_windows; ++i) {
        int rc = check_pairwise_args(ctx, m, windows[i].site_begin, windows[i].site_end, fn);
        if (rc) return rc;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    int rc = IMPOP_OK;
    // s_scope 1: s_p of every panel from the streaming scan of the same windows — one plan, its subset mask swapped per panel
    std::vector<uint32_t> sp_host;
    if (params->s_scope == 1) {
        impop_scan_params sp;
        sp.struct_size = sizeof sp; sp.d_pi_mode = params->d_pi_mode; sp.s_scope = 1; sp.tile_blocks = 0;
        impop_scan_plan *plan = nullptr;
        rc = impop_scan_plan_create(ctx, m, windows, n_windows, masks, nullptr, nullptr, &sp, &plan);
        if (rc) return rc;
        std::vector<impop_window_stats> rec(n_windows);
        sp_host.resize((size_t)K * n_windows);
        for (uint32_t k = 0; k < K && !rc; ++k) {
            rc = impop_scan_plan_set_masks(plan, masks + (size_t)k * mwords, nullptr, nullptr);
            if (!rc) rc = impop_scan_plan_launch(plan, nullptr);
            if (!rc) rc = impop_scan_plan_fetch(plan, rec.data());
            for (uint64_t i = 0; i < n_windows && !rc; ++i) sp_host[(size_t)k * n_windows + i] = rec[i].s_p;
        }
        impop_scan_plan_destroy(plan);
        if (rc) return rc;
    }
    const bool use_segmap = params->s_scope != 2;  // s_all of every window from the matrix's cached site bitmap
    if (use_segmap && (rc = ensure_segmap(ctx, m))) return rc;
    PanelEpilogue epi;
    epi.params = params; epi.n = n; epi.K = K; epi.NP = out_pairs ? K * (K - 1) / 2 : 0u;
    epi.idx = &idx; epi.sizes = &sizes; epi.cls = &cls; epi.sp_host = params->s_scope == 1 ? &sp_host : nullptr;
    epi.n_windows = n_windows; epi.out_panels = out_panels; epi.out_pairs = out_pairs; epi.out_windows = out_windows;
    PairFront in{};
    in.fn = fn; in.identity_kind = params->identity_kind; in.round_digits = params->round_digits;
    in.scan_host = nullptr; in.use_segmap = use_segmap;
    in.epi_fixed = PanelEpilogue::fixed_bytes(n, K); in.epi_per_window = PanelEpilogue::window_bytes(K, epi.NP);
    in.out_per_window = PanelEpilogue::staged_bytes(K, epi.NP);
    return pairwise_front(ctx, m, windows, n_windows, in, epi);
}

IMPOP_API int impop_pairwise_scan(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows,
                                  const uint64_t *mask_p, const uint64_t *mask_a, const uint64_t *mask_b,
                                  const impop_pairwise_params *params, impop_pairwise_stats *out_host) {
    REQUIRE(ctx && m && params, "impop_pairwise_scan: NULL argument");
    REQUIRE(params->struct_size == sizeof(impop_pairwise_params), "impop_pairwise_params.struct_size mismatch");
    REQUIRE(params->identity_kind == IMPOP_IDENTITY_MATCH || params->identity_kind == IMPOP_IDENTITY_DICE,
            "impop_pairwise_scan: unknown identity kind");
    REQUIRE(params->round_digits <= 19, "impop_pairwise_scan: round_digits > 19 unsupported");
    REQUIRE(params->d_pi_mode >= 0 && params->d_pi_mode <= 2 && params->s_scope >= 0 && params->s_scope <= 2,
            "impop_pairwise_scan: bad d_pi_mode / s_scope");
    REQUIRE(params->fst_method <= 1, "impop_pairwise_scan: fst_method must be 0 (direct) or 1 (grouped)");
    if (!n_windows) return IMPOP_OK;
    REQUIRE(windows && out_host, "impop_pairwise_scan: NULL windows/out");
    for (uint64_t i = 0; i < n_windows; ++i) {
        int rc = check_pairwise_args(ctx, m, windows[i].site_begin, windows[i].site_end, "impop_pairwise_scan");
        if (rc) return rc;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    const uint32_t n = m->g.n_hap;
    // integer S / W of the same windows from the streaming scan
    impop_scan_params sp;
    sp.struct_size = sizeof sp; sp.d_pi_mode = params->d_pi_mode; sp.s_scope = params->s_scope; sp.tile_blocks = 0;
    // s_scope 2: the caller does not need S / Tajima's D (pica2- or Fst-only output): skip the site scan
    const bool want_s = params->s_scope != 2;
    if (!want_s) sp.s_scope = 0;
    // without a subset mask S comes from the matrix's cached site bitmap (s_p = s_all); with one, s_p needs the
    // subset's own counts: the streaming scan of the same windows
    const bool use_segmap = want_s && !mask_p;
    impop_scan_plan *plan = nullptr;
    int rc = (want_s && !use_segmap) ? impop_scan_plan_create(ctx, m, windows, n_windows, mask_p, mask_a, mask_b, &sp, &plan) : IMPOP_OK;
    if (rc) return rc;
    auto fail = [&](int code) {
        if (plan) impop_scan_plan_destroy(plan);
        return code;
    };
    if (use_segmap) {
        rc = ensure_segmap(ctx, m);
        if (rc) return fail(rc);
    }
    // subset P index list and A/B flags
    std::vector<uint32_t> idx;
    std::vector<uint8_t> fa(n, 0), fb(n, 0);
    for (uint32_t i = 0; i < n; ++i) {
        const bool inP = mask_p ? ((mask_p[i >> 6] >> (i & 63)) & 1ull) : true;
        if (inP) idx.push_back(i);
        fa[i] = mask_a ? (uint8_t)((mask_a[i >> 6] >> (i & 63)) & 1ull) : 0;
        fb[i] = mask_b ? (uint8_t)((mask_b[i >> 6] >> (i & 63)) & 1ull) : 0;
    }
    const uint32_t nP = (uint32_t)idx.size();
    std::vector<uint32_t> ia, ib;  // hud.py grouped: members of A / B with the overlap removed from both
    for (uint32_t i = 0; i < n && params->fst_method == 1; ++i) {
        if (fa[i] && !fb[i]) ia.push_back(i);
        if (fb[i] && !fa[i]) ib.push_back(i);
    }
    std::vector<impop_window_stats> scan_host;  // only with a scan plan; else the records are n_sites and zeros (S: the device fills it in)
    if (plan) {
        scan_host.resize(n_windows);
        rc = impop_scan_plan_launch(plan, nullptr);
        if (rc) return fail(rc);
        rc = impop_scan_plan_fetch(plan, scan_host.data());
        if (rc) return fail(rc);
    }
    PairwiseStatsEpilogue epi;
    epi.params = params; epi.mask_p = mask_p; epi.n = n; epi.nP = nP; epi.want_s = want_s;
    epi.idx = &idx; epi.ia = &ia; epi.ib = &ib; epi.fa = &fa; epi.fb = &fb; epi.out_host = out_host;
    PairFront in{};
    in.fn = "impop_pairwise_scan"; in.identity_kind = params->identity_kind; in.round_digits = params->round_digits;
    in.scan_host = plan ? scan_host.data() : nullptr; in.use_segmap = use_segmap;
    in.epi_fixed = PairwiseStatsEpilogue::fixed_bytes(n); in.epi_per_window = PairwiseStatsEpilogue::window_bytes();
    in.out_per_window = sizeof(impop_pairwise_stats);
    return fail(pairwise_front(ctx, m, windows, n_windows, in, epi));
}

IMPOP_API int impop_cluster_scan(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows,
                                 const uint64_t *mask_p, const impop_cluster_params *params, impop_cluster_stats *out_host,
                                 uint32_t *cluster_of, uint32_t *sizes) {
    REQUIRE(ctx && m && params, "impop_cluster_scan: NULL argument");
    REQUIRE(params->struct_size == sizeof(impop_cluster_params), "impop_cluster_params.struct_size mismatch");
    REQUIRE(params->identity_kind == IMPOP_IDENTITY_MATCH || params->identity_kind == IMPOP_IDENTITY_DICE,
            "impop_cluster_scan: unknown identity kind");
    REQUIRE(params->round_digits <= 19, "impop_cluster_scan: round_digits > 19 unsupported");
    // subset P index list
    const uint32_t n = m->g.n_hap;
    std::vector<uint32_t> idx;
    for (uint32_t i = 0; i < n; ++i)
        if (mask_p ? ((mask_p[i >> 6] >> (i & 63)) & 1ull) : true) idx.push_back(i);
    const uint32_t nP = (uint32_t)idx.size();
    // refused before anything is uploaded or launched
    REQUIRE(nP <= IMPOP_CLUSTER_MAX_N, "impop_cluster_scan: %u members exceed the LDS-resident clustering limit (%u)", nP,
            (uint32_t)IMPOP_CLUSTER_MAX_N);
    if (!n_windows) return IMPOP_OK;
    REQUIRE(windows && out_host, "impop_cluster_scan: NULL windows/out");
    for (uint64_t i = 0; i < n_windows; ++i) {
        int rc = check_pairwise_args(ctx, m, windows[i].site_begin, windows[i].site_end, "impop_cluster_scan");
        if (rc) return rc;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    ClusterEpilogue epi;
    epi.params = params; epi.mask_p = mask_p; epi.nP = nP; epi.idx = &idx; epi.out_host = out_host;
    epi.cluster_of = cluster_of; epi.sizes = sizes;
    uint64_t call_max_W = 0;
    for (uint64_t i = 0; i < n_windows; ++i) call_max_W = std::max(call_max_W, window_W(m, windows[i].site_begin, windows[i].site_end));
    epi.adj_bytes = af_small_certain(params->identity_kind, nP, m->n_hap_pad, call_max_W) ? 0 : af_adjacency_bytes(nP);
    PairFront in{};
    in.fn = "impop_cluster_scan"; in.identity_kind = params->identity_kind; in.round_digits = params->round_digits;
    in.scan_host = nullptr; in.use_segmap = false;  // the site scan for S / D is not needed (impop_pairwise_scan's s_scope 2)
    in.epi_fixed = ClusterEpilogue::fixed_bytes(nP); in.epi_per_window = epi.window_bytes();
    in.out_per_window = sizeof(impop_cluster_stats) + (epi.want_members() ? 2 * (size_t)nP * 4 : 0);
    // the general form keeps a window's adjacency rows in memory (20 MB at the limit): chunks of at most 2 GiB of them
    in.max_chunk_windows = std::min<uint64_t>(65535, std::max<uint64_t>(1, (2ull << 30) / std::max<size_t>(in.epi_per_window, 1)));
    return pairwise_front(ctx, m, windows, n_windows, in, epi);
}
