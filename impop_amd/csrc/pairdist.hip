// pairdist.hip — impop_pairdist_scan: its distribution kernel, its PairEpilogue (pair_front.h) and the entry point.  Per window,
// from the chunk's Gram counts, the sums, extremes and histograms of the pairwise distances inside K panels and between their pairs,
// and every member's nearest neighbours against each panel, then the records.  All combines and the finalisation are pairdist_math.h.
//
// One workgroup per window; the panels' haplotype indexes and the Gram diagonal sit in LDS.  A wave owns a ROW: member p against
// every other member q, panel by panel (the members are laid out panel-major, so a panel is a range of positions).  The Gram
// kernel writes the upper triangle only, so the entry of (p, q) is read at (min, max) of the two haplotype indexes: the part of
// the row right of the diagonal is read along a Gram row, the part left of it STRIDED down a Gram column out of L2 — the choice
// made here against updating both endpoints of a triangle entry: a row then has one owner, its (min, ties) against each panel is
// one pass with a plain merge and needs no atomic minimum and no second look for the ties.  Every entry is read twice for it.
// The pairs a record counts are the q > p of a row; a wave keeps them in its lanes across its rows of one panel, reduces them once
// per pair of panels and adds the result to the record's accumulator in LDS with integer atomics.  The (min, ties) tables, M x K
// entries per window, live in global scratch.
#include "pair_front.h"

namespace impop {

constexpr int PD_T = 256;

struct PairdistTables : PanelTables {};  // a PanelTables under the name pairdist_kernel's exported symbol carries; adds nothing
struct PairdistOut {
    DistNN *nn;                              // scratch: n_problems x M x K
    impop_dist_panel *panels;                // n_problems x K
    impop_dist_pair *pairs;                  // n_problems x K (K - 1) / 2
    uint32_t *hist_within, *hist_between;    // bins > 0: n_problems x K x bins | x K (K - 1) / 2 x bins; zeroed unless hist_lds
    uint32_t bins, width;
};
constexpr size_t PAIRDIST_LDS_BYTES = 65536;     // what a workgroup takes at most: the fixed tables, and the histograms where they fit

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}
__device__ __forceinline__ DistNN wave_nn(DistNN v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        DistNN o;
        o.min_h = __shfl_xor(v.min_h, off, 64);
        o.ties = __shfl_xor(v.ties, off, 64);
        v = pd_nn_merge(v, o);
    }
    return v;
}

template <bool HIST_LDS>
__global__ __launch_bounds__(PD_T) void pairdist_kernel(SimBatch batch, const impop_window_stats *__restrict__ ws, PairdistTables T,
                                                        PairdistOut O) {
    extern __shared__ uint64_t pd_smem[];
    const uint32_t K = T.K, M = T.M, NP = K * (K - 1) / 2, R = K + NP, B = O.bins;
    DistAcc *acc = reinterpret_cast<DistAcc *>(pd_smem);   // R records' accumulators: panels, then pairs
    uint32_t *diag = reinterpret_cast<uint32_t *>(acc + R);  // a_p per position
    uint32_t *hap = diag + M;                              // haplotype index per position
    uint32_t *lh = hap + M;                                // HIST_LDS: R x B counters
    const uint64_t w = blockIdx.x;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, n_waves = PD_T / 64;
    const SimView S = sim_view(batch, w);
    const bool no_sites = S.W == 0;  // every H is 0
    for (uint32_t r = tid; r < R; r += PD_T) acc[r] = pd_acc_empty();
    for (uint32_t p = tid; p < M; p += PD_T) {
        const uint32_t h = T.hap_of[p];
        hap[p] = h;
        diag[p] = no_sites ? 0u : (uint32_t)gram_at(S, h, h);
    }
    if (HIST_LDS)
        for (uint32_t i = tid; i < R * B; i += PD_T) lh[i] = 0;
    __syncthreads();
    uint32_t *hw = O.hist_within + w * (uint64_t)K * B, *hb = O.hist_between + w * (uint64_t)NP * B;
    DistNN *nn = O.nn + w * (uint64_t)M * K;

    // rows of panel cp against panel c: the record is fixed, so a lane keeps its sums and keys across the wave's rows and the wave
    // reduces them once per (cp, c); only a row's (min, ties) is reduced per row
    for (uint32_t cp = 0; cp < K; ++cp)
        for (uint32_t c = 0; c < K; ++c) {
            const uint32_t lo = T.off[c], hi = T.off[c + 1];
            const bool counted = c >= cp;  // panels before the row's own hold only q < p: nearest neighbours alone
            const uint32_t rec = c == cp ? c : K + pd_pair_index(K, cp < c ? cp : c, cp < c ? c : cp);
            DistAcc a = pd_acc_empty();
            for (uint32_t p = T.off[cp] + wave; p < T.off[cp + 1]; p += n_waves) {
                const uint32_t hp = hap[p], ap = diag[p];
                DistNN mine = pd_nn_empty();
                for (uint32_t q = lo + lane; q < hi; q += 64) {
                    if (q == p) continue;
                    const uint32_t hq = hap[q];
                    uint32_t H = 0;
                    if (!no_sites) H = ap + diag[q] - 2u * (uint32_t)gram_at(S, hp < hq ? hp : hq, hp < hq ? hq : hp);
                    pd_nn_add(mine, H);
                    if (counted && q > p) {
                        pd_acc_add(a, H, p, q);
                        if (B) {
                            const uint32_t bin = pd_bin(H, O.width, B);
                            if (HIST_LDS) atomicAdd(&lh[rec * B + bin], 1u);
                            else atomicAdd(rec < K ? &hw[rec * B + bin] : &hb[(rec - K) * B + bin], 1u);
                        }
                    }
                }
                mine = wave_nn(mine);
                if (lane == 0) nn[(uint64_t)p * K + c] = mine;
            }
            if (counted) {
                a.sum_h = wave_sum_u64(a.sum_h); a.sum_h2 = wave_sum_u64(a.sum_h2); a.n_zero = wave_sum_u64(a.n_zero);
                a.min_key = wave_min_u64(a.min_key); a.max_key = wave_max_u64(a.max_key);
                if (lane == 0 && a.max_key != PD_MAX_EMPTY) {
                    atomicAdd(reinterpret_cast<unsigned long long *>(&acc[rec].sum_h), (unsigned long long)a.sum_h);
                    atomicAdd(reinterpret_cast<unsigned long long *>(&acc[rec].sum_h2), (unsigned long long)a.sum_h2);
                    atomicAdd(reinterpret_cast<unsigned long long *>(&acc[rec].n_zero), (unsigned long long)a.n_zero);
                    atomicMin(reinterpret_cast<unsigned long long *>(&acc[rec].min_key), (unsigned long long)a.min_key);
                    atomicMax(reinterpret_cast<unsigned long long *>(&acc[rec].max_key), (unsigned long long)a.max_key);
                }
            }
        }
    __threadfence_block();  // the (min, ties) tables were written by other waves of this workgroup
    __syncthreads();

    const uint32_t n_sites = ws[w].n_sites;
    if (tid < K) {
        const uint64_t m = T.off[tid + 1] - T.off[tid], n_pairs = m * (m - 1) / 2;
        const DistFields f = pd_fields(acc[tid], n_pairs, hap);
        impop_dist_panel r;
        r.n_members = (uint32_t)m; r.n_sites = n_sites; r.n_pairs = n_pairs;
        r.sum_h = f.sum_h; r.sum_h2 = f.sum_h2; r.n_zero = f.n_zero;
        r.min_h = f.min_h; r.max_h = f.max_h; r.min_i = f.min_i; r.min_j = f.min_j; r.max_i = f.max_i; r.max_j = f.max_j;
        O.panels[w * K + tid] = r;
    }
    for (uint32_t pr = wave; pr < NP; pr += n_waves) {
        const PanelPair P = panel_pair(K, T.merged, T.moff, pr);
        const uint32_t ka = P.ka, kb = P.kb, len = P.len, *list = P.list;  // the positions of ka u kb in ascending haplotype index
        double sum = 0.0;
        uint32_t same_a = 0, same_b = 0, other_a = 0, other_b = 0;
        for (uint32_t base = 0; base < len; base += 64) {
            const uint32_t i = base + lane;
            double term = 0.0;
            if (i < len) {
                const uint32_t pos = list[i];
                const bool in_a = pos < T.off[ka + 1];
                uint32_t tied, same;
                pd_nn_pair(nn[(uint64_t)pos * K + (in_a ? ka : kb)], nn[(uint64_t)pos * K + (in_a ? kb : ka)], &tied, &same);
                term = pd_snn_term(same, tied);
                if (same == tied) (in_a ? same_a : same_b) += 1;
                if (same == 0) (in_a ? other_a : other_b) += 1;
            }
            const uint32_t here = len - base < 64u ? len - base : 64u;
            for (uint32_t t = 0; t < here; ++t) sum += __shfl(term, (int)t, 64);  // one fixed order: the members in turn
        }
        same_a = wave_sum_u32(same_a); same_b = wave_sum_u32(same_b);
        other_a = wave_sum_u32(other_a); other_b = wave_sum_u32(other_b);
        if (lane == 0) {
            const uint64_t n_pairs = (uint64_t)(T.off[ka + 1] - T.off[ka]) * (T.off[kb + 1] - T.off[kb]);
            const DistFields f = pd_fields(acc[K + pr], n_pairs, hap);
            impop_dist_pair r;
            r.n_pairs = n_pairs; r.sum_h = f.sum_h; r.sum_h2 = f.sum_h2; r.n_zero = f.n_zero;
            r.min_h = f.min_h; r.max_h = f.max_h; r.min_i = f.min_i; r.min_j = f.min_j; r.max_i = f.max_i; r.max_j = f.max_j;
            r.nn_same_a = same_a; r.nn_same_b = same_b; r.nn_other_a = other_a; r.nn_other_b = other_b;
            r.snn = pd_snn_finish(sum, len);
            r.gmin = pd_gmin(f.min_h, f.sum_h, n_pairs);
            r.reserved = 0;
            O.pairs[w * NP + pr] = r;
        }
    }
    if (HIST_LDS)
        for (uint32_t i = tid; i < R * B; i += PD_T) {
            const uint32_t rec = i / B, bin = i - rec * B;
            if (rec < K) hw[rec * B + bin] = lh[i];
            else hb[(rec - K) * B + bin] = lh[i];
        }
}

// bytes of the accumulators, the diagonal and the haplotype indexes
static size_t pairdist_lds_fixed(uint32_t K, uint32_t M) { return (size_t)(K + K * (K - 1) / 2) * sizeof(DistAcc) + (size_t)M * 8; }

static int launch_pairdist(impop_ctx *ctx, const SimBatch &b, uint64_t n_problems, const impop_window_stats *d_stats, const PairdistTables &T,
                           const PairdistOut &O, bool hist_lds) {
    if (!n_problems) return IMPOP_OK;
    const uint32_t R = T.K + T.K * (T.K - 1) / 2;
    const size_t lds = pairdist_lds_fixed(T.K, T.M) + (hist_lds ? (size_t)R * O.bins * 4 : 0);
    REQUIRE(lds <= PAIRDIST_LDS_BYTES && T.M >= 1 && T.M <= PAIRDIST_MAX_N && T.K >= 1 && T.K <= 8, "launch_pairdist: bad shape");
    if (hist_lds)
        hipLaunchKernelGGL(pairdist_kernel<true>, dim3((uint32_t)n_problems), dim3(PD_T), lds, ctx->stream, b, d_stats, T, O);
    else
        hipLaunchKernelGGL(pairdist_kernel<false>, dim3((uint32_t)n_problems), dim3(PD_T), lds, ctx->stream, b, d_stats, T, O);
    HIP_TRY(hipGetLastError());
    return IMPOP_OK;
}

// impop_pairdist_scan's epilogue: one launch of the distribution kernel per chunk — records, histograms and the per-member
// nearest-neighbour tables it keeps in scratch
struct PairdistEpilogue final : PairEpilogue {
    uint32_t K, NP, M, B, width;            // B = 0: no histograms
    bool hist_lds = false;
    PairdistTables T{};
    PanelUpload tables;
    Result<impop_dist_panel> pan;
    Result<impop_dist_pair> pair;
    Result<uint32_t> hw, hb;                // hist_within, hist_between
    uint64_t launches = 0;
    DistNN *d_nn = nullptr;
    // the device bytes layout() takes per window of a chunk, histograms included (they bound a chunk: impop_pairdist_scan)
    size_t per_window_bytes() const {
        return (size_t)M * K * sizeof(DistNN) + K * sizeof(impop_dist_panel) + NP * sizeof(impop_dist_pair) + (size_t)(K + NP) * B * 4;
    }
    void layout(Layout &D, Layout &H, uint64_t cap) override {
        tables.layout(D);
        D.sub(d_nn, cap * M * K); pan.layout(D, H, cap); pair.layout(D, H, cap, NP);
        hw.layout(D, H, cap, (size_t)K * B); hb.layout(D, H, cap, (size_t)NP * B);  // one region: zeroed by one memset where the kernel tallies into it
    }
    int upload(impop_ctx *ctx) override { return tables.upload(ctx, T); }
    int launch(impop_ctx *ctx, const PairChunk &c) override {
        // the distribution kernel between two events of its own: impop_ctx_pairdist_elapsed
        int rc = timed(ctx, ctx->timers[impop_ctx::T_PAIRDIST], [&] {
            if (B && !hist_lds) HIP_TRY(hipMemsetAsync(hw.d, 0, (size_t)((char *)(hb.d + c.cnt * NP * B) - (char *)hw.d), ctx->stream));
            const PairdistOut O{d_nn, pan.d, pair.d, hw.d, hb.d, B, width};
            return launch_pairdist(ctx, c.b, c.cnt, c.d_s, T, O, hist_lds);
        });
        if (rc) return rc;
        ++launches;
        if ((rc = pan.down(ctx, c.cnt)) || (rc = pair.down(ctx, c.cnt)) || (rc = hw.down(ctx, c.cnt))) return rc;
        return hb.down(ctx, c.cnt);
    }
    void collect(const PairChunk &c) override { pan.scatter(c); pair.scatter(c); hw.scatter(c); hb.scatter(c); }
};

}  // namespace impop

using namespace impop;

static_assert(sizeof(impop_dist_panel) == 64 && sizeof(impop_dist_pair) == 96 && sizeof(impop_pairdist_params) == 16, "fixed record layouts");
static_assert(IMPOP_PAIRDIST_MAX_N == PAIRDIST_MAX_N, "positions are packed into 12 bits of a key");

IMPOP_API int impop_pairdist_scan(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows,
                                  const uint64_t *masks, uint32_t n_pop, const impop_pairdist_params *params,
                                  impop_dist_panel *out_panels, impop_dist_pair *out_pairs, uint32_t *hist_within, uint32_t *hist_between) {
    const char *fn = "impop_pairdist_scan";
    REQUIRE(ctx && m && params, "%s: NULL argument", fn);
    REQUIRE(params->struct_size == sizeof(impop_pairdist_params), "impop_pairdist_params.struct_size mismatch");
    REQUIRE(params->hist_bins <= IMPOP_PAIRDIST_MAX_BINS, "%s: hist_bins must be 0..%u", fn, (uint32_t)IMPOP_PAIRDIST_MAX_BINS);
    REQUIRE(params->hist_width >= 1, "%s: hist_width must be at least 1", fn);
    REQUIRE(n_pop >= 1 && n_pop <= 8, "%s: n_pop must be 1..8", fn);
    REQUIRE(masks, "%s: masks is NULL", fn);
    const uint32_t K = n_pop, NP = K * (K - 1) / 2;
    PanelSet panels;
    int rc = panel_refused(panel_set(masks, K, m->g.n_hap, panels), fn);
    if (rc) return rc;
    if (panels.M > IMPOP_PAIRDIST_MAX_N) {  // refused before anything is uploaded or launched
        set_error("%s: the panels hold %zu members, more than the limit of %u", fn, (size_t)panels.M, (uint32_t)IMPOP_PAIRDIST_MAX_N);
        return IMPOP_E_UNSUPPORTED;
    }
    bool go;
    if ((rc = windows_ready(ctx, m, windows, n_windows, out_panels, fn, &go)) || !go) return rc;
    const MergedPairs pairs = merged_pairs(panels, false);
    uint64_t p_max = 0;  // the pairs of the largest record
    for (uint32_t a = 0; a < K; ++a) {
        const uint64_t ma = panels.size(a);
        p_max = std::max(p_max, ma * (ma - 1) / 2);
        for (uint32_t b = a + 1; b < K; ++b) p_max = std::max(p_max, ma * panels.size(b));
    }
    const uint64_t max_W = widest_W(m, windows, n_windows);
    if (!pd_sum_h2_admitted(max_W, p_max)) {  // before any launch
        set_error("%s: sum_h2 may overflow 64 bits: the widest window has W = %llu and the largest record %llu pairs (W^2 x pairs must stay "
                  "below 2^64)", fn, (unsigned long long)max_W, (unsigned long long)p_max);
        return IMPOP_E_UNSUPPORTED;
    }
    PairdistEpilogue epi;
    epi.K = K; epi.NP = NP; epi.M = panels.M;
    epi.B = (hist_within || (hist_between && NP)) ? params->hist_bins : 0u;
    epi.width = params->hist_width;
    epi.tables.set = &panels; epi.tables.pairs = &pairs;
    epi.pan.want(out_panels, K); epi.pair.want(out_pairs, NP);
    epi.hw.want(hist_within, (size_t)K * epi.B); epi.hb.want(hist_between, (size_t)NP * epi.B);
    // histograms in LDS where every counter fits next to the kernel's tables; IMPOP_PAIRDIST_LDS_BINS=n lowers what the LDS form
    // takes, so that tests reach the global form at small sizes
    if (epi.B) {
        const size_t fixed = pairdist_lds_fixed(K, epi.M);
        size_t cap = fixed < PAIRDIST_LDS_BYTES ? (PAIRDIST_LDS_BYTES - fixed) / 4 : 0;
        const char *e = getenv("IMPOP_PAIRDIST_LDS_BINS");
        if (e && *e) {
            const long v = strtol(e, nullptr, 10);
            cap = std::min<size_t>(cap, v < 0 ? 0 : (size_t)v);
        }
        epi.hist_lds = (size_t)(K + NP) * epi.B <= cap;
    }
    // the per-member tables and the histograms of a chunk: at most 512 MiB of them
    PairFront in = hamming_front(fn, max_W, chunk_windows(512ull << 20, epi.per_window_bytes()));
    rc = pairwise_front(ctx, m, windows, n_windows, in, epi);
    if (rc) return rc;
    if (trace_on())
        fprintf(stderr, "[impop_pairdist_scan] pops=%u pairs=%u members=%u windows=%llu chunks=%llu launches=%llu hist_bins=%u hist=%s\n", K, NP,
                epi.M, (unsigned long long)n_windows, (unsigned long long)in.chunks, (unsigned long long)epi.launches, epi.B,
                !epi.B ? "off" : epi.hist_lds ? "lds" : "global");
    return IMPOP_OK;
}
