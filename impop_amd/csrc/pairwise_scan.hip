// pairwise_scan.hip — the front end of the windowed all-pairs calls (pair_front.h): windows -> Gram cells -> chunks (pair_plan.h),
// per chunk the Gram launch (pairwise.hip) and the filled SimBatch, handed to the call's PairEpilogue; the steps the entry points
// share; and the three calls whose kernels are the shared statistics kernels of stats_kernels.h: impop_pairwise_scan,
// impop_pairwise_scan_panel and impop_cluster_scan.  (impop_pairdist_scan, impop_pca_scan, impop_kinship_scan and
// impop_permtest_scan sit next to their kernels: pairdist.hip, pca.hip, kinship.hip, permtest.hip.)
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "pair_front.h"
#include "pair_plan.h"

namespace impop {

// ---- record arithmetic shared by the two finalize kernels ----------------------------------------------------------
// Tajima's D of a record from its pi (as d_pi_mode selects it), S and the constants a1,a2,b1,b2,c1,c2,e1,e2 for nP sequences
__device__ __forceinline__ double record_tajima_d(const Pica2Out &p, uint32_t n_sites, double S, uint32_t nP, int d_pi_mode,
                                                  const double *__restrict__ taj) {
    const double pin = d_pi_mode == 0 ? py_round(p.pi_site, 8) : d_pi_mode == 1 ? p.pi_site : p.pi * (double)n_sites;
    if (!(nP >= 2 && pin == pin && pin >= 0)) return __builtin_nan("");
    TajConsts c;
    c.a1 = taj[0]; c.a2 = taj[1]; c.b1 = taj[2]; c.b2 = taj[3]; c.c1 = taj[4]; c.c2 = taj[5]; c.e1 = taj[6]; c.e2 = taj[7];
    return tajima_d_from(c, S, pin, nullptr, nullptr);
}
template <typename Rec>  // impop_pairwise_stats, impop_pair_stats
__device__ __forceinline__ void record_fst_fields(const HfstOut &h, Rec &r) {
    r.fst = h.v[0]; r.pi_a = h.v[1]; r.pi_b = h.v[2]; r.pi_xy = h.v[3]; r.dxy = h.v[4]; r.da = h.v[5];
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
    const impop_window_stats s = in.scan[i];
    impop_pairwise_stats r;
    r.pi = p.pi; r.pi_site = p.pi_site;
    record_fst_fields(in.hfst[i], r);
    r.n_groups = p.n_groups; r.s_all = s.s_all; r.s_p = s.s_p; r.n_sites = s.n_sites; r.reserved = 0;
    r.tajima_d = record_tajima_d(p, s.n_sites, (double)(s_scope == 0 ? s.s_all : s.s_p), nP, d_pi_mode, taj);
    out[i] = r;
}

}  // namespace impop

using namespace impop;

namespace {

// impop_pairwise_scan_panel's records from the per-panel pica2 results, the per-pair Fst results and the window's S / W: one thread
// per (window, panel or pair)
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
        impop_pair_stats r;
        record_fst_fields(in.hfst[(uint64_t)(j - K) * in.stride + w], r);
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
    r.tajima_d = s_scope != 2 ? record_tajima_d(p, s.n_sites, (double)(s_scope == 1 ? sp : s.s_all), nP, d_pi_mode, in.taj + 8 * j)
                              : __builtin_nan("");
    out_panels[w * K + j] = r;
}

// ---- the shared front end -------------------------------------------------------------------------------------------
// per-chunk metadata: the chunk's Gram cells, then one entry per window (= problem) of the chunk
struct ChunkMeta {
    GramWindow *w;            // the cells
    uint64_t *W, *L;          // W and seq_len per problem
    uint32_t *first, *count;  // its Gram matrices inside the chunk
    impop_window_stats *s;    // n_sites, and S / the scan's sums when the call asked for them
    GramWindow *sw, *ow;      // the WINDOWS in matrix coordinates | in ORIGINAL coordinates (compacted matrices)
    void layout(Layout &M, uint64_t cap) {
        M.sub(w, cap); M.sub(W, cap); M.sub(L, cap); M.sub(first, cap); M.sub(count, cap); M.sub(s, cap); M.sub(sw, cap); M.sub(ow, cap);
    }
};

}  // namespace

namespace impop {

uint64_t widest_W(const impop_matrix *m, const impop_window *windows, uint64_t n_windows) {
    uint64_t w = 0;
    for (uint64_t i = 0; i < n_windows; ++i) w = std::max(w, window_W(m, windows[i].site_begin, windows[i].site_end));
    return w;
}

int pairwise_front(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows, PairFront &in,
                   PairEpilogue &epi) {
    const uint32_t ld = m->n_hap_pad, n = m->g.n_hap;
    // IMPOP_TRACE=1: host-side phase times of this call on stderr (where a call's time goes when the kernels are short)
    const bool trace = trace_on();
    const auto t_enter = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (trace) fprintf(stderr, "[%s] %-22s +%.1f us\n", in.fn, what,
                           std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_enter).count());
    };
    // ---- plan.  compacted matrix: the contraction runs over the KEPT (variable) sites of each window; the dropped all-ones
    // sites come back as a per-window constant (SimBatch.add), the dropped all-zero sites contribute nothing
    std::vector<impop_window> mw;
    int rc = map_windows_device(ctx, m, windows, n_windows, mw);
    if (rc) return rc;
    lap("map_windows");
    PairPlan plan;
    REQUIRE(plan_cells(mw.data(), n_windows, plan), "%s: too many windows", in.fn);
    lap("cells");
    // Chunks whose cells fit the Gram scratch (<= ~8 GiB of 288): large chunks keep the persistent Gram grid's last,
    // partially filled round of tasks small next to the launch
    const size_t gram_bytes = (size_t)ld * ld * 4;
    uint64_t cap = (8ull << 30) / gram_bytes;  // (a chromosome of 50 kb windows — 4854 on chr2 — is one chunk)
    if (cap > 8192) cap = 8192;
    cap = std::min<uint64_t>(cap, std::max<uint64_t>(plan.cells.size(), n_windows));  // a short call stages (and copies) short tables
    if (cap < 1) cap = 1;
    // windows per chunk: the Gram capacity, what the epilogue's own buffers allow, and the test switch IMPOP_PAIRWISE_CHUNK
    // (windows per chunk: forces several chunks on lists far too short to need them; records must not change)
    uint64_t win_cap = cap;
    if (in.max_chunk_windows) win_cap = std::min<uint64_t>(win_cap, std::max<uint64_t>(in.max_chunk_windows, 1));
    static const uint64_t chunk_env = [] { const char *e = getenv("IMPOP_PAIRWISE_CHUNK"); return e ? strtoull(e, nullptr, 10) : 0ull; }();
    if (chunk_env) win_cap = std::min<uint64_t>(win_cap, chunk_env);
    // one cell per window: a chunk never holds more Gram matrices than windows, so the Gram and table scratch is sized for that
    // (an epilogue that allows ~100 windows per chunk would otherwise reserve room for 8192 matrices it can never fill)
    if (!plan.segmented) cap = std::min<uint64_t>(cap, win_cap);
    // ---- allocate.  per-chunk metadata: ONE contiguous region mirrored on the host, so that a chunk costs one host-to-device
    // copy (eight small pageable copies were ~0.3 ms of host time between two Gram launches); cells first: they go up on their
    // own, everything from W on in a second copy
    ChunkMeta hm, dm;  // the same tables in page-locked memory and on the device
    Layout M, Md;
    hm.layout(M, cap);
    dm.layout(Md, cap);
    const size_t meta_bytes = M.total();
    Layout E, H;  // the epilogue's device region and its page-locked results
    epi.layout(E, H, win_cap);
    int32_t *d_g;
    char *d_meta, *d_epi;
    uint32_t *d_add;
    Layout D;  // device: Gram matrices | metadata | compacted: dropped all-ones sites per window | the epilogue's own region
    D.sub(d_g, cap * (gram_bytes / 4)); D.sub(d_meta, meta_bytes); D.sub(d_add, cap); D.sub(d_epi, E.total());
    void *d = nullptr;
    rc = ctx_scratch(ctx, D.total(), &d);
    if (rc) return rc;
    D.bind(d);
    E.bind(d_epi);
    rc = epi.upload(ctx);
    if (rc) return rc;
    lap("scratch");
    // page-locked staging for the metadata going up and the results coming down (ctx_pinned)
    void *pin = nullptr;
    rc = ctx_pinned(ctx, meta_bytes + H.total(), &pin);
    if (rc) return rc;
    char *hmeta = reinterpret_cast<char *>(pin);
    memset(hmeta, 0, meta_bytes);
    M.bind(hmeta);
    Md.bind(d_meta);
    H.bind(hmeta + meta_bytes);
    std::vector<uint32_t> add_h;
    const size_t o_W = (size_t)((char *)hm.W - hmeta);  // cells go up on their own, everything from W on in a second copy
    bool g16 = false;
    // ---- per chunk
    PairChunkWalk walk(plan, cap, win_cap);
    PairChunkSpan s;
    for (PairChunkWalk::Step step; (step = walk.next(s)) != PairChunkWalk::DONE;) {
        REQUIRE(step != PairChunkWalk::TOO_WIDE, "%s: window %llu spans %u segments, more than the %llu Gram matrices that fit the scratch",
                in.fn, (unsigned long long)walk.bad_window, walk.bad_cells, (unsigned long long)cap);
        const uint64_t cnt = s.cnt, *ord = plan.ord.data() + s.base;
        uint64_t max_sites = 0;
        for (uint32_t c = 0; c < s.n_cells; ++c) {
            const PairCell &cell = plan.cells[s.c_lo + c];
            hm.w[c] = {cell.b, cell.e};
            max_sites = std::max<uint64_t>(max_sites, cell.e - cell.b);
        }
        // the Gram launch needs the cells alone: they go up first and the kernel starts, the per-window tables are filled in (and
        // copied) while it runs
        if (s.n_cells) {
            HIP_TRY(hipMemcpyAsync(dm.w, hm.w, (size_t)s.n_cells * sizeof(GramWindow), hipMemcpyHostToDevice, ctx->stream));
            // counts as uint16 where every count of the call fits (a count is at most its window's W): half the result bytes
            static const bool u16_off = env_is("IMPOP_GRAM_U16", '0');
            g16 = !u16_off && in.max_W < 65536;
            // impop_ctx_gram_timing: the Gram launch(es) of this chunk between two events
            rc = timed(ctx, ctx->timers[impop_ctx::T_GRAM], [&] { return launch_gram_any(ctx, m, dm.w, hm.w, s.n_cells, d_g, max_sites, &g16); });
            if (rc) return rc;
            if (in.identity_kind != IMPOP_IDENTITY_MATCH) {  // `match` sees Hamming distances only: polarity-invariant
                rc = launch_gram_unflip(ctx, m, d_g, s.n_cells, g16);
                if (rc) return rc;
            }
        }
        for (uint64_t k = 0; k < cnt; ++k) {
            const uint64_t wdx = ord[k];
            hm.W[k] = window_W(m, windows[wdx].site_begin, windows[wdx].site_end);
            hm.L[k] = windows[wdx].seq_len;
            hm.first[k] = s.first_of(plan, wdx);
            hm.count[k] = plan.count[wdx];
            if (in.scan_host) hm.s[k] = in.scan_host[wdx];
            else { memset(&hm.s[k], 0, sizeof(hm.s[k])); hm.s[k].n_sites = (uint32_t)hm.W[k]; }
            hm.sw[k] = {mw[wdx].site_begin, mw[wdx].site_end};
            hm.ow[k] = {windows[wdx].site_begin, windows[wdx].site_end};
        }
        const bool one_to_one = s.one_to_one(plan);
        lap("chunk metadata");
        HIP_TRY(hipMemcpyAsync(dm.W, hm.W, meta_bytes - o_W, hipMemcpyHostToDevice, ctx->stream));
        if (in.use_segmap && (rc = launch_seg_count(ctx, m->d_segmap, dm.sw, cnt, dm.s, nullptr))) return rc;
        PairChunk ch{};
        SimBatch &b = ch.b;
        b.gram = d_g; b.stride = (uint64_t)ld * ld; b.ld = ld; b.n = n; b.W = dm.W; b.kind = in.identity_kind;
        b.g16 = g16 ? 1u : 0u;
        b.max_W = in.max_W;
        b.round_digits = in.round_digits < 0 ? -1 : in.round_digits;
        b.seg_first = one_to_one ? nullptr : dm.first; b.seg_count = one_to_one ? nullptr : dm.count;
        if (compact_weighted(m)) {  // the dropped all-ones sites' summed weights, from the host prefix sums
            add_h.resize(cnt);
            for (uint64_t k = 0; k < cnt; ++k) add_h[k] = ones_weight(m, windows[ord[k]].site_begin, windows[ord[k]].site_end);
            HIP_TRY(hipMemcpyAsync(d_add, add_h.data(), cnt * 4, hipMemcpyHostToDevice, ctx->stream));
            b.add = d_add;
        } else if (m->compact) {  // ... their count, from the bitmap on the device
            if ((rc = launch_seg_count(ctx, m->d_onesmap, dm.ow, cnt, nullptr, d_add))) return rc;
            b.add = d_add;
        }
        ch.cnt = cnt; ch.ord = ord; ch.d_L = dm.L; ch.d_s = dm.s;
        ++in.chunks;
        rc = epi.launch(ctx, ch);
        if (rc) return rc;
        lap("chunk launched");
        rc = ctx_err_fetch(ctx);
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(ctx->stream));  // the staging vectors are reused by the next chunk
        rc = ctx_err_result(ctx, in.fn);  // a device-side consistency check tripped: no partial results
        if (rc) return rc;
        epi.collect(ch);
        lap("chunk done");
    }
    return IMPOP_OK;
}

int check_windows(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows, const char *fn) {
    for (uint64_t i = 0; i < n_windows; ++i) {
        const int rc = check_pairwise_args(ctx, m, windows[i].site_begin, windows[i].site_end, fn);
        if (rc) return rc;
    }
    return IMPOP_OK;
}
int windows_ready(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows, const void *out, const char *fn,
                  bool *go) {
    *go = false;
    if (!n_windows) return IMPOP_OK;
    REQUIRE(windows && out, "%s: NULL windows/out", fn);
    const int rc = check_windows(ctx, m, windows, n_windows, fn);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    *go = true;
    return IMPOP_OK;
}
int panel_refused(const PanelRefusal &r, const char *fn) {
    REQUIRE(r.kind != PanelRefusal::OVERLAP, "%s: populations must be disjoint (population %u overlaps population %u)", fn, r.k, r.other);
    REQUIRE(r.kind != PanelRefusal::EMPTY, "%s: population %u is empty", fn, r.k);
    return IMPOP_OK;
}

}  // namespace impop

namespace {

// impop_pairwise_scan's epilogue: pica2 grouping next to the Fst sums, then the fixed records
struct PairwiseStatsEpilogue final : PairEpilogue {
    const impop_pairwise_params *params;
    const uint64_t *mask_p;
    uint32_t n, nP;
    bool want_s;
    const std::vector<uint32_t> *idx, *ia, *ib;
    const std::vector<uint8_t> *fa, *fb;
    Result<impop_pairwise_stats> rec;
    Pica2Out *d_p = nullptr;
    HfstOut *d_h = nullptr;
    uint32_t *d_idx = nullptr, *d_ia = nullptr, *d_ib = nullptr;
    uint8_t *d_fa = nullptr, *d_fb = nullptr;
    void layout(Layout &D, Layout &H, uint64_t cap) override {
        const size_t n1 = n ? n : 1;
        D.sub(d_idx, n1); D.sub(d_ia, n1); D.sub(d_ib, n1); D.sub(d_fa, n1); D.sub(d_fb, n1);
        D.sub(d_h, cap); rec.layout(D, H, cap); D.sub(d_p, cap);
    }
    int upload(impop_ctx *ctx) override {
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
        int rc = on_side_stream(ctx, [&] { return launch_pica2(ctx, b, cnt, mask_p ? d_idx : nullptr, nP, nullptr, params->threshold, c.d_L, d_p, nullptr); });
        if (rc) return rc;
        if (params->fst_method == 1)
            rc = launch_hud_grouped(ctx, b, cnt, d_ia, (uint32_t)ia->size(), d_ib, (uint32_t)ib->size(), nullptr, nullptr, params->threshold,
                                    c.d_L, d_h);
        else
            rc = launch_hfst(ctx, b, cnt, d_fa, d_fb, c.d_L, d_h);
        if (rc) return rc;
        HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
        PairFinalIn in{d_p, d_h, c.d_s};
        rc = ensure_tajima_consts(ctx, nP >= 2 ? (int64_t)nP : 2);  // the cache may have been retargeted by another call
        if (rc) return rc;
        hipLaunchKernelGGL(pairwise_finalize_kernel, dim3((uint32_t)((cnt + 63) / 64)), dim3(64), 0, ctx->stream, in, cnt,
                           want_s ? nP : 0u, params->d_pi_mode, want_s ? params->s_scope : 0, ctx->d_taj, rec.d);
        HIP_TRY(hipGetLastError());
        return rec.down(ctx, cnt);
    }
    void collect(const PairChunk &c) override { rec.scatter(c); }
};

// impop_cluster_scan's epilogue: one clustering launch (stats_kernels.h launch_af_batch), records and member tables
struct ClusterEpilogue final : PairEpilogue {
    const impop_cluster_params *params;
    const uint64_t *mask_p;
    uint32_t nP;
    const std::vector<uint32_t> *idx;
    Result<impop_cluster_stats> rec;
    Result<uint32_t> cl, sz;  // cluster_of, sizes
    size_t adj_bytes = 0;  // per window: the general form's adjacency rows (0 when the call is sure to take the window-shape kernel)
    uint32_t *d_idx = nullptr;
    char *d_adj = nullptr;
    bool want_members() const { return cl.out || sz.out; }
    // the window-shape kernel writes tables only when asked; the general form always writes both (sizes is its ranking's output)
    size_t table_words() const { return (adj_bytes == 0 && !want_members()) ? 0 : nP; }
    // the device bytes layout() takes per window of a chunk (they bound a chunk: impop_cluster_scan)
    size_t per_window_bytes() const { return sizeof(impop_cluster_stats) + 2 * table_words() * 4 + adj_bytes; }
    void layout(Layout &D, Layout &H, uint64_t cap) override {
        D.sub(d_idx, nP ? nP : 1);
        rec.layout(D, H, cap); cl.layout(D, H, cap, table_words()); sz.layout(D, H, cap, table_words()); D.sub(d_adj, cap * adj_bytes);
    }
    int upload(impop_ctx *ctx) override {
        if (nP) HIP_TRY(hipMemcpyAsync(d_idx, idx->data(), (size_t)nP * 4, hipMemcpyHostToDevice, ctx->stream));
        return IMPOP_OK;
    }
    int launch(impop_ctx *ctx, const PairChunk &c) override {
        // the clustering kernel(s) between two events of their own: impop_ctx_cluster_elapsed
        int rc = timed(ctx, ctx->timers[impop_ctx::T_CLUSTER], [&] {
            return launch_af_batch(ctx, c.b, c.cnt, mask_p ? d_idx : nullptr, nP, params->threshold, reinterpret_cast<uint32_t *>(d_adj), adj_bytes,
                                   rec.d, cl.d, sz.d, want_members());
        });
        if (rc || (rc = rec.down(ctx, c.cnt)) || (rc = cl.down(ctx, c.cnt))) return rc;
        return sz.down(ctx, c.cnt);
    }
    void collect(const PairChunk &c) override { rec.scatter(c); cl.scatter(c); sz.scatter(c); }
};

// impop_pairwise_scan_panel's epilogue: K panels and their K (K - 1) / 2 pairs on the chunk's ONE set of Gram matrices — pica2 per
// panel on the side stream, next to it the Fst sums of all pairs (one launch of hfst_panel_small_kernel on the window-statistics
// shape; launch_hfst per pair on every other), then the records
struct PanelEpilogue final : PairEpilogue {
    const impop_pairwise_params *params;
    uint32_t n, K, NP;                      // NP = 0: no pair records asked for
    const std::vector<uint32_t> *idx, *sizes;  // the panels' members back to back, each ascending | members per panel
    const std::vector<uint8_t> *cls;        // class of haplotype i, 0xFF: none
    const std::vector<uint32_t> *sp_host;   // s_scope 1: K x n_windows, panel-major; else nullptr
    uint64_t n_windows;
    Result<impop_panel_stats> pan;
    Result<impop_pair_stats> pair;
    Result<impop_panel_window> win;  // comes down whether or not the caller passed an array: n = 1 either way
    bool traced = false;
    uint64_t cap = 0;  // windows per chunk the buffers are laid out for: panel k (pair p) of problem w at k * cap + w
    Pica2Out *d_p = nullptr;
    HfstOut *d_h = nullptr;
    uint32_t *d_idx = nullptr, *d_sizes = nullptr, *d_sp = nullptr;
    uint8_t *d_cls = nullptr, *d_flags = nullptr;  // d_flags: K x n membership flags (the general route's in_a / in_b)
    double *d_taj = nullptr;
    std::vector<uint32_t> sp_chunk;
    std::vector<uint8_t> flags_host;
    void layout(Layout &D, Layout &H, uint64_t cap_) override {
        cap = cap_;
        const size_t n1 = n ? n : 1;
        D.sub(d_idx, n1); D.sub(d_sizes, K); D.sub(d_taj, (size_t)K * 8); D.sub(d_cls, n1); D.sub(d_flags, (size_t)K * n1);
        D.sub(d_p, cap * K); D.sub(d_h, cap * NP); pan.layout(D, H, cap); pair.layout(D, H, cap); win.layout(D, H, cap); D.sub(d_sp, cap * K);
    }
    int upload(impop_ctx *ctx) override {
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
    int launch(impop_ctx *ctx, const PairChunk &c) override {
        const SimBatch &b = c.b;
        const uint64_t cnt = c.cnt;
        const bool small = hfst_panel_small_applies(b);
        if (!traced && trace_on())
            fprintf(stderr, "[impop_pairwise_scan_panel] pops=%u pairs=%u route=%s\n", K, K * (K - 1) / 2, small ? "small" : "general");
        traced = true;
        if (sp_host) {  // s_scope 1: the chunk's rows of the streaming scan's s_p, in the chunk's problem order
            sp_chunk.resize((size_t)K * cap);
            for (uint32_t k = 0; k < K; ++k)
                for (uint64_t i = 0; i < cnt; ++i) sp_chunk[(size_t)k * cap + i] = (*sp_host)[(size_t)k * n_windows + c.ord[i]];
            HIP_TRY(hipMemcpyAsync(d_sp, sp_chunk.data(), (size_t)K * cap * 4, hipMemcpyHostToDevice, ctx->stream));
        }
        int rc = on_side_stream(ctx, [&] {
            int r = IMPOP_OK;
            for (uint32_t k = 0, at = 0; k < K && !r; at += (*sizes)[k], ++k)
                r = launch_pica2(ctx, b, cnt, d_idx + at, (*sizes)[k], nullptr, params->threshold, c.d_L, d_p + (uint64_t)k * cap, nullptr);
            return r;
        });
        if (rc) return rc;
        if (NP) {
            // impop_ctx_gram_timing: the Fst kernel(s) of the chunk between two events (impop_ctx_cluster_elapsed)
            rc = timed(ctx, ctx->timers[impop_ctx::T_CLUSTER], [&] {
                if (small) return launch_hfst_panel_small(ctx, b, cnt, d_cls, K, c.d_L, d_h, cap);
                int r = IMPOP_OK;
                uint32_t p = 0;
                for (uint32_t a = 0; a < K && !r; ++a)
                    for (uint32_t bb = a + 1; bb < K && !r; ++bb, ++p)
                        r = launch_hfst(ctx, b, cnt, d_flags + (size_t)a * n, d_flags + (size_t)bb * n, c.d_L, d_h + (uint64_t)p * cap);
                return r;
            });
            if (rc) return rc;
        }
        HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
        PanelFinalIn in{d_p, NP ? d_h : nullptr, c.d_s, sp_host ? d_sp : nullptr, d_taj, d_sizes, cap};
        const uint64_t items = cnt * (K + NP);
        hipLaunchKernelGGL(panel_finalize_kernel, dim3((uint32_t)((items + 127) / 128)), dim3(128), 0, ctx->stream, in, cnt, K,
                           params->d_pi_mode, params->s_scope, pan.d, pair.d, win.d);
        HIP_TRY(hipGetLastError());
        if ((rc = pan.down(ctx, cnt)) || (rc = pair.down(ctx, cnt))) return rc;
        return win.down(ctx, cnt);
    }
    void collect(const PairChunk &c) override { pan.scatter(c); pair.scatter(c); win.scatter(c); }
};

// the checks of impop_pairwise_params common to the calls that take one
int check_pairwise_params(const impop_pairwise_params *params, const char *fn) {
    REQUIRE(params->struct_size == sizeof(impop_pairwise_params), "impop_pairwise_params.struct_size mismatch");
    REQUIRE(params->identity_kind == IMPOP_IDENTITY_MATCH || params->identity_kind == IMPOP_IDENTITY_DICE, "%s: unknown identity kind", fn);
    REQUIRE(params->round_digits <= 19, "%s: round_digits > 19 unsupported", fn);
    REQUIRE(params->d_pi_mode >= 0 && params->d_pi_mode <= 2 && params->s_scope >= 0 && params->s_scope <= 2, "%s: bad d_pi_mode / s_scope", fn);
    return IMPOP_OK;
}

}  // namespace
static_assert(sizeof(impop_panel_stats) == 48 && sizeof(impop_panel_window) == 8 && sizeof(impop_pair_stats) == 48, "fixed record layouts");

IMPOP_API int impop_pairwise_scan_panel(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows,
                                        const uint64_t *masks, uint32_t n_pop, const impop_pairwise_params *params,
                                        impop_panel_stats *out_panels, impop_pair_stats *out_pairs, impop_panel_window *out_windows) {
    const char *fn = "impop_pairwise_scan_panel";
    REQUIRE(ctx && m && params, "%s: NULL argument", fn);
    int rc = check_pairwise_params(params, fn);
    if (rc) return rc;
    REQUIRE(params->fst_method <= 1, "%s: fst_method must be 0 (direct)", fn);
    if (params->fst_method == 1) {
        set_error("%s: fst_method 1 (hud.py grouped) is not available for panels; use impop_pairwise_scan per pair", fn);
        return IMPOP_E_UNSUPPORTED;
    }
    REQUIRE(n_pop >= 2 && n_pop <= 8, "%s: n_pop must be 2..8", fn);
    REQUIRE(masks, "%s: masks is NULL", fn);
    const uint32_t n = m->g.n_hap, K = n_pop, mwords = (n + 63) / 64;
    // disjoint: h-fst.py:181-185 removes shared members per pair, which would make a panel's size depend on the pair
    PanelSet panels;
    if ((rc = panel_refused(panel_set(masks, K, n, panels), fn))) return rc;
    bool go;
    if ((rc = windows_ready(ctx, m, windows, n_windows, out_panels, fn, &go)) || !go) return rc;
    // s_scope 1: s_p of every panel from the streaming scan of the same windows — one plan, its subset mask swapped per panel
    std::vector<uint32_t> sp_host;
    if (params->s_scope == 1) {
        impop_scan_params sp;
        sp.struct_size = sizeof sp; sp.d_pi_mode = params->d_pi_mode; sp.s_scope = 1; sp.tile_blocks = 0;
        impop_scan_plan *plan = nullptr;
        rc = scan_plan_create(ctx, m, windows, n_windows, masks, nullptr, nullptr, &sp, false, &plan);
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
    epi.idx = &panels.hap_of; epi.sizes = &panels.sizes; epi.cls = &panels.cls; epi.sp_host = params->s_scope == 1 ? &sp_host : nullptr;
    epi.n_windows = n_windows;
    epi.pan.want(out_panels, K); epi.pair.want(out_pairs, epi.NP); epi.win.out = out_windows; epi.win.n = 1;
    PairFront in = front_params(fn, params->identity_kind, params->round_digits, widest_W(m, windows, n_windows));
    in.use_segmap = use_segmap;
    return pairwise_front(ctx, m, windows, n_windows, in, epi);
}

IMPOP_API int impop_pairwise_scan(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows,
                                  const uint64_t *mask_p, const uint64_t *mask_a, const uint64_t *mask_b,
                                  const impop_pairwise_params *params, impop_pairwise_stats *out_host) {
    const char *fn = "impop_pairwise_scan";
    REQUIRE(ctx && m && params, "%s: NULL argument", fn);
    int rc = check_pairwise_params(params, fn);
    if (rc) return rc;
    REQUIRE(params->fst_method <= 1, "%s: fst_method must be 0 (direct) or 1 (grouped)", fn);
    bool go;
    if ((rc = windows_ready(ctx, m, windows, n_windows, out_host, fn, &go)) || !go) return rc;
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
    rc = (want_s && !use_segmap) ? scan_plan_create(ctx, m, windows, n_windows, mask_p, mask_a, mask_b, &sp, false, &plan) : IMPOP_OK;
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
    const std::vector<uint32_t> idx = mask_members(mask_p, n);
    std::vector<uint8_t> fa(n, 0), fb(n, 0);
    if (mask_a) for (uint32_t i : mask_members(mask_a, n)) fa[i] = 1;
    if (mask_b) for (uint32_t i : mask_members(mask_b, n)) fb[i] = 1;
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
    epi.idx = &idx; epi.ia = &ia; epi.ib = &ib; epi.fa = &fa; epi.fb = &fb; epi.rec.want(out_host, 1);
    PairFront in = front_params(fn, params->identity_kind, params->round_digits, widest_W(m, windows, n_windows));
    in.scan_host = plan ? scan_host.data() : nullptr; in.use_segmap = use_segmap;
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
    const std::vector<uint32_t> idx = mask_members(mask_p, m->g.n_hap);  // subset P index list
    const uint32_t nP = (uint32_t)idx.size();
    // refused before anything is uploaded or launched
    REQUIRE(nP <= IMPOP_CLUSTER_MAX_N, "impop_cluster_scan: %u members exceed the LDS-resident clustering limit (%u)", nP,
            (uint32_t)IMPOP_CLUSTER_MAX_N);
    bool go;
    const int rc = windows_ready(ctx, m, windows, n_windows, out_host, "impop_cluster_scan", &go);
    if (rc || !go) return rc;
    ClusterEpilogue epi;
    epi.params = params; epi.mask_p = mask_p; epi.nP = nP; epi.idx = &idx;
    epi.rec.want(out_host, 1); epi.cl.want(cluster_of, nP); epi.sz.want(sizes, nP);
    // no segmap: the site scan for S / D is not needed (impop_pairwise_scan's s_scope 2)
    PairFront in = front_params("impop_cluster_scan", params->identity_kind, params->round_digits, widest_W(m, windows, n_windows));
    epi.adj_bytes = af_small_certain(params->identity_kind, nP, m->n_hap_pad, in.max_W) ? 0 : af_adjacency_bytes(nP);
    // the general form keeps a window's adjacency rows in memory (20 MB at the limit): chunks of at most 2 GiB of them
    in.max_chunk_windows = chunk_windows(2ull << 30, epi.per_window_bytes());
    return pairwise_front(ctx, m, windows, n_windows, in, epi);
}
