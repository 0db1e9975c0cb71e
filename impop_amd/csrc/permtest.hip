// permtest.hip — the two kernels of impop_permtest_scan (pairwise_scan.hip PermtestEpilogue): permutation p-values for Hudson's
// Fst, AMOVA Phi_ST, Dxy and S_nn per window and pair of panels.  All comparisons and the (wa, wb) algebra are perm_math.h.
//
// Preparation, one workgroup per (window, pair): a wave owns a ROW i of the pair's distance matrix H (the members of both panels in
// ascending haplotype index), reads the Gram counts as pairdist.hip does and writes the row into scratch as BYTE PLANES: plane q
// holds ((H >> 8q) & 255) - 128 as int8, row-major with a row stride of m_pad = 64 ceil(m / 64).  Entries at or beyond m are never
// initialised: they only ever meet a zero of Z.  From the same registers the wave takes the row sum r_i, the row's share of the
// observed wa / wb, d_i, the tie mask T_i (one ballot per 64 columns IS one word of the mask), tied_i and same_i(z0).
//
// Labelling kernel, one workgroup per (window, pair, block of 63 labellings): its 64 columns are z0 and 63 labellings, 16 per
// wave.  Y = H Z on the matrix cores (v_mfma_i32_16x16x64_i8, A = a 16 x 64 tile of a plane, B = 64 x 16 of Z expanded from the bit
// masks in registers), one pass over the planes; the accumulator tile is masked by z and summed over its rows at once, so Y is never
// stored.  Lane l carries row l & 15 of A and column l & 15 of B, both for the k-group l >> 4, byte j of A against byte j of B: the
// result does not depend on which k the hardware gives a (group, byte), only on A and B agreeing, which they do by construction.
// With s = byte - 128, sum_ij z_i s_ij z_j = z^T H_q z - 128 m_a^2 for every column with m_a ones.  S_nn runs next to it in the VALU.
// Column 0 of every task is z0: its (wa, wb, nn) must equal the preparation kernel's direct values, else DEV_ERR_PERMTEST.
#include "perm_math.h"
#include "stats_kernels.h"

namespace impop {

constexpr int PT_T = 256;

typedef int pt_i32x4 __attribute__((ext_vector_type(4)));

struct PermPair {
    uint32_t ka, kb, m, m_k, mw, m_pad;
    const uint32_t *list;
};
__device__ __forceinline__ PermPair perm_pair(const PermtestTables &T, uint32_t pr) {
    PermPair P;
    uint32_t ka = 0, rest = pr;
    while (rest >= T.K - 1 - ka) { rest -= T.K - 1 - ka; ++ka; }
    P.ka = ka; P.kb = ka + 1 + rest;
    P.list = T.merged + T.moff[pr];
    P.m = T.moff[pr + 1] - T.moff[pr];
    P.m_k = T.off[ka + 1] - T.off[ka];
    P.mw = (P.m + 63) / 64;
    P.m_pad = P.mw * 64;
    return P;
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(PT_T) void permtest_prep_kernel(SimBatch batch, PermtestTables T, PermtestScratch X) {
    __shared__ uint32_t hap[PERMTEST_MAX_N], diag[PERMTEST_MAX_N];
    __shared__ uint64_t z0l[PERMTEST_MAX_N / 64];
    __shared__ unsigned long long acc[4];  // 2 tot, 2 wa, 2 wb, nn
    const uint64_t slot = blockIdx.x, w = slot / T.NP;
    const uint32_t pr = (uint32_t)(slot % T.NP);
    const PermPair P = perm_pair(T, pr);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, m = P.m, mw = P.mw;
    const SimView S = sim_view(batch, w);
    const bool no_sites = S.W == 0;
    for (uint32_t i = tid; i < m; i += PT_T) {
        const uint32_t h = T.hap_of[P.list[i]];
        hap[i] = h;
        diag[i] = no_sites ? 0u : (uint32_t)gram_at(S, h, h);
    }
    if (tid < mw) z0l[tid] = T.z0[(uint64_t)pr * T.mw_max + tid];
    if (tid < 4) acc[tid] = 0;
    __syncthreads();
    const uint64_t plane_bytes = (uint64_t)T.m_pad_max * T.m_pad_max;
    int8_t *planes = X.planes + slot * plane_bytes * T.planes;
    uint64_t *ties = X.ties + slot * (uint64_t)T.m_pad_max * T.mw_max;
    uint64_t *rows = X.rows + slot * T.m_pad_max;
    uint32_t *term = X.term + slot * T.m_pad_max, *st = X.st + slot * T.m_pad_max;
    for (uint32_t i = wave; i < m; i += PT_T / 64) {
        const uint32_t hi = hap[i], ai = diag[i];
        const bool zi = perm_bit(z0l, i);
        uint32_t hv[PERMTEST_MAX_N / 64];
        uint64_t rsum = 0, ssum = 0;  // the row's sum | its part over the members with i's own label
        uint32_t mn = 0xFFFFFFFFu;
#pragma unroll
        for (uint32_t t = 0; t < PERMTEST_MAX_N / 64; ++t) {
            hv[t] = 0;
            if (t < mw) {
                const uint32_t j = t * 64 + lane;
                if (j < m) {
                    uint32_t h = 0;
                    if (j != i && !no_sites) {
                        const uint32_t hj = hap[j];
                        h = ai + diag[j] - 2u * (uint32_t)gram_at(S, hi < hj ? hi : hj, hi < hj ? hj : hi);
                    }
                    hv[t] = h;
                    for (uint32_t q = 0; q < T.planes; ++q)
                        planes[q * plane_bytes + (uint64_t)i * P.m_pad + j] = (int8_t)((int)((h >> (8 * q)) & 255u) - 128);
                    if (j != i) {
                        rsum += h;
                        if ((bool)((z0l[t] >> lane) & 1ull) == zi) ssum += h;
                        mn = h < mn ? h : mn;
                    }
                }
            }
        }
        mn = wave_min_u32(mn);
        uint32_t tied = 0, same = 0;
#pragma unroll
        for (uint32_t t = 0; t < PERMTEST_MAX_N / 64; ++t)
            if (t < mw) {
                const uint32_t j = t * 64 + lane;
                const uint64_t word = __ballot(j < m && j != i && hv[t] == mn);
                if (lane == 0) ties[(uint64_t)i * mw + t] = word;
                tied += (uint32_t)__popcll(word);
                same += (uint32_t)__popcll(word & (zi ? z0l[t] : ~z0l[t]));
            }
        rsum = wave_sum_u64(rsum);
        ssum = wave_sum_u64(ssum);
        if (lane == 0) {
            const uint32_t tm = perm_nn_term(tied);
            rows[i] = rsum; term[i] = tm; st[i] = same << 16 | tied;
            atomicAdd(&acc[0], (unsigned long long)rsum);
            atomicAdd(&acc[zi ? 1 : 2], (unsigned long long)ssum);
            atomicAdd(&acc[3], (unsigned long long)same * tm);
        }
    }
    __syncthreads();
    if (tid == 0) X.obs[slot] = PermObs{acc[1] / 2, acc[2] / 2, acc[3], acc[0] / 2};
}

// the 16 bits b of a k-group as 16 bytes of 0 / 1: every nibble times 0x00204081 puts bit s at bit 8 s (no two products meet)
__device__ __forceinline__ pt_i32x4 perm_expand16(uint32_t b) {
    pt_i32x4 v;
    v.x = (int)(((b & 15u) * 0x00204081u) & 0x01010101u);
    v.y = (int)((((b >> 4) & 15u) * 0x00204081u) & 0x01010101u);
    v.z = (int)((((b >> 8) & 15u) * 0x00204081u) & 0x01010101u);
    v.w = (int)((((b >> 12) & 15u) * 0x00204081u) & 0x01010101u);
    return v;
}
__device__ __forceinline__ int64_t group_sum_i64(int64_t v) {  // over the four lane groups of a column
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

__global__ __launch_bounds__(PT_T) void permtest_label_kernel(PermtestTables T, PermtestScratch X, uint32_t n_blk, uint32_t *err) {
    __shared__ uint64_t zl[PERM_TASK_COLS][PERMTEST_MAX_N / 64];
    const uint64_t task = blockIdx.x, slot = task / n_blk;
    const uint32_t blk = (uint32_t)(task % n_blk), pr = (uint32_t)(slot % T.NP);
    const PermPair P = perm_pair(T, pr);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, m = P.m, mw = P.mw, m_pad = P.m_pad;
    const uint64_t *labels = T.labels + T.loff[pr];
    for (uint32_t e = tid; e < PERM_TASK_COLS * mw; e += PT_T) {
        const uint32_t c = e / mw, t = e - c * mw;
        const uint32_t r = blk * (PERM_TASK_COLS - 1) + c - 1;  // column 0: z0
        zl[c][t] = c == 0 ? T.z0[(uint64_t)pr * T.mw_max + t] : r < T.n_perm ? labels[(uint64_t)r * mw + t] : 0ull;
    }
    __syncthreads();
    const uint64_t plane_bytes = (uint64_t)T.m_pad_max * T.m_pad_max;
    const int8_t *planes = X.planes + slot * plane_bytes * T.planes;
    const uint64_t *ties = X.ties + slot * (uint64_t)T.m_pad_max * T.mw_max;
    const uint64_t *rows = X.rows + slot * T.m_pad_max;
    const uint32_t *term = X.term + slot * T.m_pad_max;
    const uint32_t col = wave * 16 + (lane & 15u), g = lane >> 4;
    const uint64_t *z = zl[col];

    // z^T H z: the planes in turn, per plane the 16-row tiles in turn
    int64_t zHz = 0;
    for (uint32_t q = 0; q < T.planes; ++q) {
        const int8_t *pl = planes + q * plane_bytes;
        int32_t cs = 0;  // this lane's rows of the masked column sum: |.| <= 1024 rows x 1024 x 128
        for (uint32_t rt = 0; rt < m_pad / 16; ++rt) {
            pt_i32x4 c4 = {0, 0, 0, 0};
            const int8_t *arow = pl + (uint64_t)(rt * 16 + (lane & 15u)) * m_pad + g * 16;
            for (uint32_t ks = 0; ks < mw; ++ks) {
                const pt_i32x4 a = *reinterpret_cast<const pt_i32x4 *>(arow + ks * 64);
                const pt_i32x4 b = perm_expand16((uint32_t)(z[ks] >> (16 * g)) & 0xFFFFu);
                c4 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c4, 0, 0, 0);
            }
            const uint32_t row0 = rt * 16 + g * 4;  // C/D: column lane & 15, rows 4 (lane >> 4) + reg
            const uint32_t zb = (uint32_t)(z[row0 >> 6] >> (row0 & 63u));
            cs += (zb & 1u ? c4.x : 0) + (zb & 2u ? c4.y : 0) + (zb & 4u ? c4.z : 0) + (zb & 8u ? c4.w : 0);
        }
        zHz += (int64_t)cs * ((int64_t)1 << (8 * q));
    }
    // z^T r and nn: this lane takes the rows i = g mod 4 of its column
    int64_t zr = 0, nn = 0;
    for (uint32_t i = g; i < m; i += 4) {
        const bool zi = perm_bit(z, i);
        if (zi) zr += (int64_t)rows[i];
        uint32_t same = 0;
        for (uint32_t t = 0; t < mw; ++t) same += (uint32_t)__popcll(ties[(uint64_t)i * mw + t] & (zi ? z[t] : ~z[t]));
        nn += (int64_t)((uint64_t)same * term[i]);
    }
    zHz = group_sum_i64(zHz);
    zr = group_sum_i64(zr);
    nn = group_sum_i64(nn);
    int64_t ones = 0;  // the 128 a row's ones took off every product, per plane
    for (uint32_t q = 0; q < T.planes; ++q) ones += (int64_t)1 << (8 * q);
    zHz += 128 * (int64_t)P.m_k * P.m_k * ones;

    const PermObs o = X.obs[slot];
    uint64_t wa, wb;
    perm_wa_wb((uint64_t)zHz, (uint64_t)zr, 2 * o.tot, &wa, &wb);
    const uint32_t r = blk * (PERM_TASK_COLS - 1) + col - 1;
    const bool owner = g == 0 && col != 0 && r < T.n_perm;
    if (g == 0 && col == 0 && (wa != o.wa || wb != o.wb || (uint64_t)nn != o.nn)) atomicOr(err, DEV_ERR_PERMTEST);
    const uint64_t m_l = m - P.m_k;
    const uint64_t f0 = __ballot(owner && perm_ge_fst(wa, wb, o, P.m_k, m_l));
    const uint64_t f1 = __ballot(owner && perm_ge_phi(wa, wb, o, P.m_k, m_l));
    const uint64_t f2 = __ballot(owner && perm_ge_dxy(wa, wb, o));
    const uint64_t f3 = __ballot(owner && perm_ge_snn((uint64_t)nn, o));
    if (lane == 0) {
        uint32_t *ge = X.ge + slot * 4;
        if (f0) atomicAdd(&ge[0], (uint32_t)__popcll(f0));
        if (f1) atomicAdd(&ge[1], (uint32_t)__popcll(f1));
        if (f2) atomicAdd(&ge[2], (uint32_t)__popcll(f2));
        if (f3) atomicAdd(&ge[3], (uint32_t)__popcll(f3));
    }
    if (owner && X.null) {
        uint64_t *e = X.null + (slot * T.n_perm + r) * 3;
        e[0] = wa; e[1] = wb; e[2] = (uint64_t)nn;
    }
}

uint32_t permtest_blocks(uint32_t n_perm) { return (n_perm + PERM_TASK_COLS - 2) / (PERM_TASK_COLS - 1); }

int launch_permtest_prep(impop_ctx *ctx, const SimBatch &b, uint64_t n_problems, const PermtestTables &T, const PermtestScratch &X) {
    if (!n_problems) return IMPOP_OK;
    REQUIRE(T.K >= 2 && T.K <= 8 && T.M >= 2 && T.M <= PERMTEST_MAX_N && T.planes >= 1 && T.planes <= 4 && T.m_pad_max == 64 * T.mw_max &&
                T.mw_max <= PERMTEST_MAX_N / 64 && n_problems * T.NP < 0x7FFFFFFFull, "launch_permtest_prep: bad shape");
    hipLaunchKernelGGL(permtest_prep_kernel, dim3((uint32_t)(n_problems * T.NP)), dim3(PT_T), 0, ctx->stream, b, T, X);
    HIP_TRY(hipGetLastError());
    return IMPOP_OK;
}

int launch_permtest_labels(impop_ctx *ctx, uint64_t n_problems, const PermtestTables &T, const PermtestScratch &X) {
    if (!n_problems) return IMPOP_OK;
    const uint32_t n_blk = permtest_blocks(T.n_perm);
    REQUIRE(T.n_perm >= 1 && T.n_perm <= PERMTEST_MAX_PERM && n_problems * T.NP * n_blk < 0x7FFFFFFFull, "launch_permtest_labels: bad shape");
    hipLaunchKernelGGL(permtest_label_kernel, dim3((uint32_t)(n_problems * T.NP * n_blk)), dim3(PT_T), 0, ctx->stream, T, X, n_blk, ctx->d_err);
    HIP_TRY(hipGetLastError());
    return IMPOP_OK;
}

}  // namespace impop
