// permtest.hip — impop_permtest_scan: its two kernels, its PairEpilogue (pair_front.h) and the entry points.  Permutation p-values
// for Hudson's Fst, AMOVA Phi_ST, Dxy and S_nn per window and pair of panels.  All comparisons and the (wa, wb) algebra are perm_math.h.
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
#include "pair_front.h"
#include "perm_math.h"

namespace impop {

constexpr int PT_T = 256;

// A SLOT is a (problem, pair of panels): slot = problem x NP + pair.  The members of a pair are positions 0 .. m - 1 in ascending
// haplotype index (the merged lists of panel_set.h); m_pad = 64 ceil(m / 64).
constexpr uint32_t PERM_TASK_COLS = 64;  // columns of a labelling task: z0 and 63 labellings
struct PermtestTables {
    PanelTables P;
    const uint64_t *z0;       // per pair p: the observed labelling, mw_max words at p x mw_max
    const uint64_t *labels;   // per pair p: n_perm x ceil(m_p / 64) words at loff[p]
    const uint64_t *loff;     // NP
    uint32_t NP, n_perm, planes, m_pad_max, mw_max;  // planes: bytes of a distance, 1..4; the largest m_pad / its words
};
struct PermtestScratch {
    int8_t *planes;    // slot x planes x m_pad_max^2: plane q of H as (byte - 128), row stride the PAIR's m_pad
    uint64_t *ties;    // slot x m_pad_max x mw_max: row i's nearest-neighbour tie mask at i x ceil(m / 64)
    uint64_t *rows;    // slot x m_pad_max: r_i
    uint32_t *term;    // slot x m_pad_max: SCALE / tied_i
    uint32_t *st;      // slot x m_pad_max: same_i(z0) << 16 | tied_i (the host's snn)
    PermObs *obs;      // slot: the observed wa, wb, nn and tot
    uint32_t *ge;      // slot x 4: fst, phi, dxy, snn; zeroed by the caller, added to with integer atomics
    uint64_t *null;    // slot x n_perm x {wa, wb, nn}, or nullptr
};

typedef int pt_i32x4 __attribute__((ext_vector_type(4)));

struct PermPair : PanelPair {
    uint32_t m, m_k, mw, m_pad;
};
__device__ __forceinline__ PermPair perm_pair(const PermtestTables &T, uint32_t pr) {
    PermPair P;
    static_cast<PanelPair &>(P) = panel_pair(T.P.K, T.P.merged, T.P.moff, pr);
    P.m = P.len;
    P.m_k = T.P.off[P.ka + 1] - T.P.off[P.ka];
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
        const uint32_t h = T.P.hap_of[P.list[i]];
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

// labelling tasks per slot
static uint32_t permtest_blocks(uint32_t n_perm) { return (n_perm + PERM_TASK_COLS - 2) / (PERM_TASK_COLS - 1); }

static int launch_permtest_prep(impop_ctx *ctx, const SimBatch &b, uint64_t n_problems, const PermtestTables &T, const PermtestScratch &X) {
    if (!n_problems) return IMPOP_OK;
    REQUIRE(T.P.K >= 2 && T.P.K <= 8 && T.P.M >= 2 && T.P.M <= PERMTEST_MAX_N && T.planes >= 1 && T.planes <= 4 && T.m_pad_max == 64 * T.mw_max &&
                T.mw_max <= PERMTEST_MAX_N / 64 && n_problems * T.NP < 0x7FFFFFFFull, "launch_permtest_prep: bad shape");
    hipLaunchKernelGGL(permtest_prep_kernel, dim3((uint32_t)(n_problems * T.NP)), dim3(PT_T), 0, ctx->stream, b, T, X);
    HIP_TRY(hipGetLastError());
    return IMPOP_OK;
}

static int launch_permtest_labels(impop_ctx *ctx, uint64_t n_problems, const PermtestTables &T, const PermtestScratch &X) {
    if (!n_problems) return IMPOP_OK;
    const uint32_t n_blk = permtest_blocks(T.n_perm);
    REQUIRE(T.n_perm >= 1 && T.n_perm <= PERMTEST_MAX_PERM && n_problems * T.NP * n_blk < 0x7FFFFFFFull, "launch_permtest_labels: bad shape");
    hipLaunchKernelGGL(permtest_label_kernel, dim3((uint32_t)(n_problems * T.NP * n_blk)), dim3(PT_T), 0, ctx->stream, T, X, n_blk, ctx->d_err);
    HIP_TRY(hipGetLastError());
    return IMPOP_OK;
}

// impop_permtest_scan's epilogue: per chunk the preparation kernel (byte planes of every pair's distance matrix, row sums, tie
// masks, the observed integers) and the labelling kernel (the null integers on the matrix cores, compared and counted on the
// device); the doubles of a record are finalised here, on the host, from the integers (perm_math.h)
struct PermtestEpilogue final : PairEpilogue {
    PermtestTables T{};
    PanelUpload tables;
    uint32_t n_perm;
    const std::vector<uint64_t> *labels, *loff;
    impop_perm_pair *out_pairs;
    uint64_t launches = 0;
    uint64_t *d_z0 = nullptr, *d_labels = nullptr, *d_loff = nullptr;
    PermtestScratch X{};
    Result<uint32_t> st, ge;            // consumed by collect, like obs
    Result<PermObs> obs;
    Result<impop_perm_null> null;       // the one result that goes to the caller as it comes down
    impop_window_stats *h_ws = nullptr; // the front end's records of the chunk (its d_s): not a Result, there is no device buffer to list
    // the device bytes layout() takes per window of a chunk (they bound a chunk: impop_permtest_scan)
    size_t per_window_bytes() const {
        const size_t mp = T.m_pad_max;
        return (size_t)T.NP * (mp * mp * T.planes + mp * T.mw_max * 8 + mp * 16 + sizeof(PermObs) + 16 + (null.out ? (size_t)n_perm * 24 : 0));
    }
    void layout(Layout &D, Layout &H, uint64_t cap) override {
        const size_t slots = cap * T.NP, mp = T.m_pad_max;
        tables.layout(D);
        D.sub(d_z0, tables.pairs->z0.size()); D.sub(d_labels, labels->size()); D.sub(d_loff, T.NP);
        D.sub(X.planes, slots * mp * mp * T.planes); D.sub(X.ties, slots * mp * T.mw_max); D.sub(X.rows, slots * mp);
        D.sub(X.term, slots * mp); st.layout(D, H, cap); obs.layout(D, H, cap); ge.layout(D, H, cap); null.layout(D, H, cap);
        H.sub(h_ws, cap);
    }
    int upload(impop_ctx *ctx) override {
        const std::vector<uint64_t> &z0 = tables.pairs->z0;
        if (int rc = tables.upload(ctx, T.P)) return rc;
        HIP_TRY(hipMemcpyAsync(d_z0, z0.data(), z0.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(d_labels, labels->data(), labels->size() * 8, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(d_loff, loff->data(), loff->size() * 8, hipMemcpyHostToDevice, ctx->stream));
        T.z0 = d_z0; T.labels = d_labels; T.loff = d_loff;
        X.st = st.d; X.obs = obs.d; X.ge = ge.d;
        X.null = null.n ? reinterpret_cast<uint64_t *>(null.d) : nullptr;  // (a table of zero bytes shares its offset with what follows it)
        return IMPOP_OK;
    }
    int launch(impop_ctx *ctx, const PairChunk &c) override {
        const uint64_t cnt = c.cnt, slots = cnt * T.NP;
        HIP_TRY(hipMemsetAsync(X.ge, 0, slots * 16, ctx->stream));
        // the two kernels between events of their own: impop_ctx_permtest_elapsed
        int rc = timed(ctx, ctx->timers[impop_ctx::T_PERM], [&] { return launch_permtest_prep(ctx, c.b, cnt, T, X); });
        if (rc || (rc = timed(ctx, ctx->timers[impop_ctx::T_PERM + 1], [&] { return launch_permtest_labels(ctx, cnt, T, X); }))) return rc;
        launches += 2;
        if ((rc = obs.down(ctx, cnt)) || (rc = ge.down(ctx, cnt)) || (rc = st.down(ctx, cnt))) return rc;
        HIP_TRY(hipMemcpyAsync(h_ws, c.d_s, cnt * sizeof(impop_window_stats), hipMemcpyDeviceToHost, ctx->stream));
        return null.down(ctx, cnt);
    }
    void collect(const PairChunk &c) override {
        const uint32_t *off = T.P.off;
        for (uint64_t k = 0; k < c.cnt; ++k)
            for (uint32_t p = 0, a = 0; a < T.P.K; ++a)
                for (uint32_t b = a + 1; b < T.P.K; ++b, ++p) {
                    const uint64_t slot = k * T.NP + p;
                    const PermObs &o = obs.h[slot];
                    const uint32_t m_k = off[a + 1] - off[a], m_l = off[b + 1] - off[b], *g = ge.h + slot * 4;
                    const PermDoubles d = perm_doubles(o, m_k, m_l);
                    impop_perm_pair r;
                    r.n_a = m_k; r.n_b = m_l; r.n_sites = h_ws[k].n_sites; r.n_perm = n_perm;
                    r.wa = o.wa; r.wb = o.wb; r.ab = o.tot - o.wa - o.wb; r.nn = o.nn;
                    r.ge_fst = g[0]; r.ge_phi = g[1]; r.ge_dxy = g[2]; r.ge_snn = g[3];
                    r.fst = d.fst; r.phi_st = d.phi_st; r.dxy = d.dxy; r.snn = perm_snn(st.h + slot * T.m_pad_max, m_k + m_l);
                    r.p_fst = perm_p(g[0], n_perm); r.p_phi = perm_p(g[1], n_perm); r.p_dxy = perm_p(g[2], n_perm);
                    r.p_snn = perm_p(g[3], n_perm);
                    out_pairs[c.ord[k] * T.NP + p] = r;
                }
        null.scatter(c);
    }
};

}  // namespace impop

using namespace impop;

static_assert(sizeof(impop_permtest_params) == 16 && sizeof(impop_perm_pair) == 128 && sizeof(impop_perm_null) == 24, "fixed record layouts");
static_assert(IMPOP_PERMTEST_MAX_N == PERMTEST_MAX_N && IMPOP_PERMTEST_MAX_PERM == PERMTEST_MAX_PERM, "the kernels' tables are sized for these");

IMPOP_API int impop_permtest_labels(uint64_t seed, uint32_t pair_index, uint32_t m, uint32_t m_a, uint32_t n_perm, uint64_t *out) {
    const char *fn = "impop_permtest_labels";
    REQUIRE(out || !n_perm, "%s: out is NULL", fn);
    REQUIRE(m >= 2 && m <= IMPOP_PERMTEST_MAX_N && m_a >= 1 && m_a < m, "%s: needs 1 <= m_a < m <= %u", fn, (uint32_t)IMPOP_PERMTEST_MAX_N);
    REQUIRE(n_perm <= IMPOP_PERMTEST_MAX_PERM, "%s: n_perm must be at most %u", fn, (uint32_t)IMPOP_PERMTEST_MAX_PERM);
    std::vector<uint32_t> a(m);
    const uint32_t mw = (m + 63) / 64;
    for (uint32_t r = 0; r < n_perm; ++r) perm_labelling(seed, pair_index, r, m, m_a, a.data(), out + (size_t)r * mw);
    return IMPOP_OK;
}

IMPOP_API int impop_permtest_scan(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows,
                                  const uint64_t *masks, uint32_t n_pop, const impop_permtest_params *params, impop_perm_pair *out_pairs,
                                  impop_perm_null *out_null) {
    const char *fn = "impop_permtest_scan";
    REQUIRE(ctx && m && params, "%s: NULL argument", fn);
    REQUIRE(params->struct_size == sizeof(impop_permtest_params), "impop_permtest_params.struct_size mismatch");
    REQUIRE(n_pop >= 2 && n_pop <= 8, "%s: n_pop must be 2..8", fn);
    REQUIRE(params->n_perm >= 1 && params->n_perm <= IMPOP_PERMTEST_MAX_PERM, "%s: n_perm must be 1..%u", fn, (uint32_t)IMPOP_PERMTEST_MAX_PERM);
    REQUIRE(masks, "%s: masks is NULL", fn);
    const uint32_t K = n_pop, NP = K * (K - 1) / 2, n_perm = params->n_perm;
    PanelSet panels;
    int rc = panel_refused(panel_set(masks, K, m->g.n_hap, panels), fn);
    if (rc) return rc;
    if (panels.M > IMPOP_PERMTEST_MAX_N) {  // refused before anything is uploaded or launched
        set_error("%s: the panels hold %zu members, more than the limit of %u", fn, (size_t)panels.M, (uint32_t)IMPOP_PERMTEST_MAX_N);
        return IMPOP_E_UNSUPPORTED;
    }
    if (out_null && (n_windows > (1ull << 22) || n_windows * NP * n_perm > (1ull << 22))) {
        set_error("%s: a null table of %llu windows x %u pairs x %u labellings exceeds 2^22 entries", fn, (unsigned long long)n_windows, NP, n_perm);
        return IMPOP_E_UNSUPPORTED;
    }
    bool go;
    if ((rc = windows_ready(ctx, m, windows, n_windows, out_pairs, fn, &go)) || !go) return rc;
    uint64_t p_max = 0;
    for (uint32_t k = 0; k < K; ++k) p_max = std::max<uint64_t>(p_max, perm_q(panels.size(k)));
    const uint64_t max_W = widest_W(m, windows, n_windows);
    if (!perm_fst_admitted(max_W, p_max)) {  // before any launch
        set_error("%s: the Fst comparison may overflow: the widest window has W = %llu and the largest panel %llu pairs (W x pairs^2 must "
                  "stay at or below 2^62)", fn, (unsigned long long)max_W, (unsigned long long)p_max);
        return IMPOP_E_UNSUPPORTED;
    }
    // per pair of panels: the merged list with the observed labelling over it, and the labellings themselves (the one generator:
    // perm_math.h perm_labelling)
    const MergedPairs pairs = merged_pairs(panels, true);
    std::vector<uint32_t> fy(IMPOP_PERMTEST_MAX_N);
    std::vector<uint64_t> labels, loff;
    for (uint32_t a = 0, p = 0; a < K; ++a)
        for (uint32_t b = a + 1; b < K; ++b, ++p) {
            const uint32_t mp = pairs.moff[p + 1] - pairs.moff[p], mw = (mp + 63) / 64;
            loff.push_back(labels.size());
            labels.resize(labels.size() + (size_t)n_perm * mw);
            for (uint32_t r = 0; r < n_perm; ++r)
                perm_labelling(params->seed, p, r, mp, panels.size(a), fy.data(), labels.data() + loff[p] + (size_t)r * mw);
        }
    PermtestEpilogue epi;
    epi.T.NP = NP; epi.T.n_perm = n_perm;
    uint64_t h_max = max_W;  // a distance is at most its window's W; on a compacted matrix at most what the window KEEPS
    if (compact_weighted(m)) {
        h_max = 0;
        for (uint64_t i = 0; i < n_windows; ++i)
            h_max = std::max(h_max, window_W(m, windows[i].site_begin, windows[i].site_end) - ones_weight(m, windows[i].site_begin, windows[i].site_end));
    } else if (m->compact) {
        std::vector<impop_window> kept;
        if ((rc = map_windows_device(ctx, m, windows, n_windows, kept))) return rc;
        h_max = 0;
        for (uint64_t i = 0; i < n_windows; ++i) h_max = std::max(h_max, kept[i].site_end - kept[i].site_begin);
    }
    epi.T.planes = h_max < 256 ? 1u : h_max < 65536 ? 2u : h_max < (1ull << 24) ? 3u : 4u;
    epi.T.mw_max = pairs.mw_max; epi.T.m_pad_max = 64 * pairs.mw_max;
    epi.n_perm = n_perm;
    epi.tables.set = &panels; epi.tables.pairs = &pairs; epi.labels = &labels; epi.loff = &loff;
    epi.out_pairs = out_pairs;
    epi.obs.n = NP; epi.ge.n = (size_t)NP * 4; epi.st.n = (size_t)NP * epi.T.m_pad_max;
    epi.null.want(out_null, (size_t)NP * n_perm);
    // the byte planes, tie masks and null rows of a chunk: at most 1 GiB of them
    PairFront in = hamming_front(fn, max_W, chunk_windows(1ull << 30, epi.per_window_bytes()));
    rc = pairwise_front(ctx, m, windows, n_windows, in, epi);
    if (rc) return rc;
    if (trace_on())
        fprintf(stderr, "[impop_permtest_scan] route=%s pops=%u pairs=%u members=%u perms=%u planes=%u windows=%llu chunks=%llu launches=%llu "
                "null=%s\n", m->compact ? "compact" : "dense", K, NP, panels.M, n_perm, epi.T.planes, (unsigned long long)n_windows,
                (unsigned long long)in.chunks, (unsigned long long)epi.launches, out_null ? "on" : "off");
    return IMPOP_OK;
}
