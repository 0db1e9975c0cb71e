// pairwise_scan.hip — the windowed all-pairs calls (impop_pairwise_scan, impop_pairwise_scan_panel, impop_cluster_scan,
// impop_pairdist_scan, impop_kinship_scan, impop_pca_scan, impop_permtest_scan): one shared
// front end — windows -> Gram cells -> chunks (pair_plan.h), per chunk the Gram launch (pairwise.hip) and the filled SimBatch — and
// what each call does with the identities: its PairEpilogue.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "pair_plan.h"
#include "pca_math.h"
#include "perm_math.h"
#include "stats_kernels.h"
#include "win_chunks.h"

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
struct PairChunk {
    SimBatch b;               // the chunk's problems: Gram counts, W, segments, the constant of a compacted matrix
    uint64_t cnt;             // windows (= problems) of the chunk
    const uint64_t *ord;      // problem k is window ord[k] of the caller's list
    uint64_t *d_L;            // seq_len per problem
    impop_window_stats *d_s;  // per problem: n_sites, and S / the scan's sums when the call asked for them
};
struct PairEpilogue {
    virtual ~PairEpilogue() {}
    // THE list of the epilogue's buffers for chunks of up to cap windows: its device sub-buffers into D, the page-locked host
    // copies of its results into H.  The front end allocates D.total() and H.total() bytes and binds the listed pointers.
    virtual void layout(Layout &D, Layout &H, uint64_t cap) = 0;
    virtual int upload(impop_ctx *ctx) = 0;  // once, behind the binding and before the first chunk: the call's own tables
    // enqueue the chunk's kernels and the copies of its results into the host buffers (the front end then checks the device
    // error word and synchronises)
    virtual int launch(impop_ctx *ctx, const PairChunk &c) = 0;
    virtual void collect(const PairChunk &c) = 0;  // after the synchronisation: the host buffers -> the caller's arrays
};
struct PairFront {
    const char *fn;
    int identity_kind, round_digits;
    const impop_window_stats *scan_host;  // nullable: the streaming scan's records of the same windows
    bool use_segmap;                      // S of every window from the matrix's site bitmap (into d_s)
    uint64_t max_W;                       // widest_W of the call's windows
    uint64_t max_chunk_windows;           // 0 = no limit of the epilogue's own
};

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

// bounds every Gram count of a call (a cell is a window or a piece of one; compacted: + its constant)
uint64_t widest_W(const impop_matrix *m, const impop_window *windows, uint64_t n_windows) {
    uint64_t w = 0;
    for (uint64_t i = 0; i < n_windows; ++i) w = std::max(w, window_W(m, windows[i].site_begin, windows[i].site_end));
    return w;
}

int pairwise_front(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows, const PairFront &in,
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
            size_t slot = 0;  // impop_ctx_gram_timing: the Gram launch(es) of this chunk between two events
            if (ctx->gram_timing && (rc = ctx->timers[impop_ctx::T_GRAM].begin(ctx->stream, &slot))) return rc;
            // counts as uint16 where every count of the call fits (a count is at most its window's W): half the result bytes
            static const bool u16_off = env_is("IMPOP_GRAM_U16", '0');
            g16 = !u16_off && in.max_W < 65536;
            rc = launch_gram_any(ctx, m, dm.w, hm.w, s.n_cells, d_g, max_sites, &g16);
            if (rc) return rc;
            if (ctx->gram_timing && (rc = ctx->timers[impop_ctx::T_GRAM].end(ctx->stream, slot))) return rc;
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
    impop_pairwise_stats *d_o = nullptr, *h_o = nullptr;
    uint32_t *d_idx = nullptr, *d_ia = nullptr, *d_ib = nullptr;
    uint8_t *d_fa = nullptr, *d_fb = nullptr;
    void layout(Layout &D, Layout &H, uint64_t cap) override {
        const size_t n1 = n ? n : 1;
        D.sub(d_idx, n1); D.sub(d_ia, n1); D.sub(d_ib, n1); D.sub(d_fa, n1); D.sub(d_fb, n1);
        D.sub(d_h, cap); D.sub(d_o, cap); D.sub(d_p, cap);
        H.sub(h_o, cap);
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
        rc = ensure_tajima_consts(ctx, nP >= 2 ? (int64_t)nP : 2);  // the cache may have been retargeted by another plan
        if (rc) return rc;
        hipLaunchKernelGGL(pairwise_finalize_kernel, dim3((uint32_t)((cnt + 63) / 64)), dim3(64), 0, ctx->stream, in, cnt,
                           want_s ? nP : 0u, params->d_pi_mode, want_s ? params->s_scope : 0, ctx->d_taj, d_o);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h_o, d_o, cnt * sizeof(impop_pairwise_stats), hipMemcpyDeviceToHost, ctx->stream));
        return IMPOP_OK;
    }
    void collect(const PairChunk &c) override {
        for (uint64_t k = 0; k < c.cnt; ++k) out_host[c.ord[k]] = h_o[k];
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
    impop_cluster_stats *d_rec = nullptr, *h_rec = nullptr;
    uint32_t *d_idx = nullptr, *d_cl = nullptr, *d_sz = nullptr, *h_cl = nullptr, *h_sz = nullptr;
    char *d_adj = nullptr;
    bool want_members() const { return cluster_of || sizes; }
    // the window-shape kernel writes tables only when asked; the general form always writes both (sizes is its ranking's output)
    size_t table_words() const { return (adj_bytes == 0 && !want_members()) ? 0 : nP; }
    // the device bytes layout() takes per window of a chunk (they bound a chunk: impop_cluster_scan)
    size_t per_window_bytes() const { return sizeof(impop_cluster_stats) + 2 * table_words() * 4 + adj_bytes; }
    void layout(Layout &D, Layout &H, uint64_t cap) override {
        D.sub(d_idx, nP ? nP : 1);
        D.sub(d_rec, cap); D.sub(d_cl, cap * table_words()); D.sub(d_sz, cap * table_words()); D.sub(d_adj, cap * adj_bytes);
        H.sub(h_rec, cap); H.sub(h_cl, cluster_of ? cap * nP : 0); H.sub(h_sz, sizes ? cap * nP : 0);
    }
    int upload(impop_ctx *ctx) override {
        if (nP) HIP_TRY(hipMemcpyAsync(d_idx, idx->data(), (size_t)nP * 4, hipMemcpyHostToDevice, ctx->stream));
        return IMPOP_OK;
    }
    int launch(impop_ctx *ctx, const PairChunk &c) override {
        const uint64_t cnt = c.cnt;
        size_t slot = 0;  // the clustering kernel(s) between two events of their own: impop_ctx_cluster_elapsed
        int rc = ctx->gram_timing ? ctx->timers[impop_ctx::T_CLUSTER].begin(ctx->stream, &slot) : IMPOP_OK;
        if (rc) return rc;
        rc = launch_af_batch(ctx, c.b, cnt, mask_p ? d_idx : nullptr, nP, params->threshold, reinterpret_cast<uint32_t *>(d_adj), adj_bytes,
                             d_rec, d_cl, d_sz, want_members());
        if (rc) return rc;
        if (ctx->gram_timing && (rc = ctx->timers[impop_ctx::T_CLUSTER].end(ctx->stream, slot))) return rc;
        HIP_TRY(hipMemcpyAsync(h_rec, d_rec, cnt * sizeof(impop_cluster_stats), hipMemcpyDeviceToHost, ctx->stream));
        if (cluster_of && nP) HIP_TRY(hipMemcpyAsync(h_cl, d_cl, cnt * nP * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (sizes && nP) HIP_TRY(hipMemcpyAsync(h_sz, d_sz, cnt * nP * 4, hipMemcpyDeviceToHost, ctx->stream));
        return IMPOP_OK;
    }
    void collect(const PairChunk &c) override {
        for (uint64_t k = 0; k < c.cnt; ++k) {
            out_host[c.ord[k]] = h_rec[k];
            if (cluster_of && nP) memcpy(cluster_of + c.ord[k] * nP, h_cl + k * nP, (size_t)nP * 4);
            if (sizes && nP) memcpy(sizes + c.ord[k] * nP, h_sz + k * nP, (size_t)nP * 4);
        }
    }
};

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
    uint64_t cap = 0;  // windows per chunk the buffers are laid out for: panel k (pair p) of problem w at k * cap + w
    Pica2Out *d_p = nullptr;
    HfstOut *d_h = nullptr;
    impop_panel_stats *d_opan = nullptr, *h_pan = nullptr;
    impop_pair_stats *d_opair = nullptr, *h_pair = nullptr;
    impop_panel_window *d_owin = nullptr, *h_win = nullptr;
    uint32_t *d_idx = nullptr, *d_sizes = nullptr, *d_sp = nullptr;
    uint8_t *d_cls = nullptr, *d_flags = nullptr;  // d_flags: K x n membership flags (the general route's in_a / in_b)
    double *d_taj = nullptr;
    std::vector<uint32_t> sp_chunk;
    std::vector<uint8_t> flags_host;
    void layout(Layout &D, Layout &H, uint64_t cap_) override {
        cap = cap_;
        const size_t n1 = n ? n : 1;
        D.sub(d_idx, n1); D.sub(d_sizes, K); D.sub(d_taj, (size_t)K * 8); D.sub(d_cls, n1); D.sub(d_flags, (size_t)K * n1);
        D.sub(d_p, cap * K); D.sub(d_h, cap * NP); D.sub(d_opan, cap * K); D.sub(d_opair, cap * NP); D.sub(d_owin, cap); D.sub(d_sp, cap * K);
        H.sub(h_pan, cap * K); H.sub(h_pair, cap * NP); H.sub(h_win, cap);
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
            size_t slot = 0;  // impop_ctx_gram_timing: the Fst kernel(s) of the chunk between two events (impop_ctx_cluster_elapsed)
            if (ctx->gram_timing && (rc = ctx->timers[impop_ctx::T_CLUSTER].begin(ctx->stream, &slot))) return rc;
            if (small) {
                rc = launch_hfst_panel_small(ctx, b, cnt, d_cls, K, c.d_L, d_h, cap);
            } else {
                uint32_t p = 0;
                for (uint32_t a = 0; a < K && !rc; ++a)
                    for (uint32_t bb = a + 1; bb < K && !rc; ++bb, ++p)
                        rc = launch_hfst(ctx, b, cnt, d_flags + (size_t)a * n, d_flags + (size_t)bb * n, c.d_L, d_h + (uint64_t)p * cap);
            }
            if (rc) return rc;
            if (ctx->gram_timing && (rc = ctx->timers[impop_ctx::T_CLUSTER].end(ctx->stream, slot))) return rc;
        }
        HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
        PanelFinalIn in{d_p, NP ? d_h : nullptr, c.d_s, sp_host ? d_sp : nullptr, d_taj, d_sizes, cap};
        const uint64_t items = cnt * (K + NP);
        hipLaunchKernelGGL(panel_finalize_kernel, dim3((uint32_t)((items + 127) / 128)), dim3(128), 0, ctx->stream, in, cnt, K,
                           params->d_pi_mode, params->s_scope, d_opan, d_opair, d_owin);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h_pan, d_opan, cnt * K * sizeof(impop_panel_stats), hipMemcpyDeviceToHost, ctx->stream));
        if (NP) HIP_TRY(hipMemcpyAsync(h_pair, d_opair, cnt * NP * sizeof(impop_pair_stats), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(h_win, d_owin, cnt * sizeof(impop_panel_window), hipMemcpyDeviceToHost, ctx->stream));
        return IMPOP_OK;
    }
    void collect(const PairChunk &c) override {
        for (uint64_t k = 0; k < c.cnt; ++k) {
            memcpy(out_panels + c.ord[k] * K, h_pan + k * K, (size_t)K * sizeof(impop_panel_stats));
            if (NP) memcpy(out_pairs + c.ord[k] * NP, h_pair + k * NP, (size_t)NP * sizeof(impop_pair_stats));
            if (out_windows) out_windows[c.ord[k]] = h_win[k];
        }
    }
};

// impop_pairdist_scan's epilogue: one launch of the distribution kernel (pairdist.hip) per chunk — records, histograms and the
// per-member nearest-neighbour tables it keeps in scratch
struct PairdistEpilogue final : PairEpilogue {
    uint32_t K, NP, M, B, width;            // B = 0: no histograms
    bool hist_lds = false;
    PairdistTables T{};
    const std::vector<uint32_t> *hap_of, *merged, *moff;
    impop_dist_panel *out_panels;
    impop_dist_pair *out_pairs;             // nullable
    uint32_t *hist_within, *hist_between;   // nullable
    uint64_t chunks = 0, launches = 0;
    uint32_t *d_hap = nullptr, *d_merged = nullptr, *d_moff = nullptr, *d_hw = nullptr, *d_hb = nullptr, *h_hw = nullptr, *h_hb = nullptr;
    DistNN *d_nn = nullptr;
    impop_dist_panel *d_pan = nullptr, *h_pan = nullptr;
    impop_dist_pair *d_pair = nullptr, *h_pair = nullptr;
    // the device bytes layout() takes per window of a chunk, histograms included (they bound a chunk: impop_pairdist_scan)
    size_t per_window_bytes() const {
        return (size_t)M * K * sizeof(DistNN) + K * sizeof(impop_dist_panel) + NP * sizeof(impop_dist_pair) + (size_t)(K + NP) * B * 4;
    }
    void layout(Layout &D, Layout &H, uint64_t cap) override {
        D.sub(d_hap, M); D.sub(d_merged, merged->size() ? merged->size() : 1); D.sub(d_moff, NP + 1);
        D.sub(d_nn, cap * M * K); D.sub(d_pan, cap * K); D.sub(d_pair, cap * NP);
        D.sub(d_hw, cap * K * B); D.sub(d_hb, cap * NP * B);  // one region: zeroed by one memset where the kernel tallies into it
        H.sub(h_pan, cap * K); H.sub(h_pair, out_pairs ? cap * NP : 0);
        H.sub(h_hw, hist_within ? cap * K * B : 0); H.sub(h_hb, hist_between ? cap * NP * B : 0);
    }
    int upload(impop_ctx *ctx) override {
        HIP_TRY(hipMemcpyAsync(d_hap, hap_of->data(), (size_t)M * 4, hipMemcpyHostToDevice, ctx->stream));
        if (!merged->empty()) HIP_TRY(hipMemcpyAsync(d_merged, merged->data(), merged->size() * 4, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(d_moff, moff->data(), (size_t)(NP + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
        T.hap_of = d_hap; T.merged = d_merged; T.moff = d_moff;
        return IMPOP_OK;
    }
    int launch(impop_ctx *ctx, const PairChunk &c) override {
        const uint64_t cnt = c.cnt;
        size_t slot = 0;  // the distribution kernel between two events of its own: impop_ctx_pairdist_elapsed
        int rc = ctx->gram_timing ? ctx->timers[impop_ctx::T_PAIRDIST].begin(ctx->stream, &slot) : IMPOP_OK;
        if (rc) return rc;
        if (B && !hist_lds)
            HIP_TRY(hipMemsetAsync(d_hw, 0, (size_t)((char *)(d_hb + cnt * NP * B) - (char *)d_hw), ctx->stream));
        PairdistOut O{d_nn, d_pan, d_pair, d_hw, d_hb, B, width};
        rc = launch_pairdist(ctx, c.b, cnt, c.d_s, T, O, hist_lds);
        if (rc) return rc;
        if (ctx->gram_timing && (rc = ctx->timers[impop_ctx::T_PAIRDIST].end(ctx->stream, slot))) return rc;
        ++chunks; ++launches;
        HIP_TRY(hipMemcpyAsync(h_pan, d_pan, cnt * K * sizeof(impop_dist_panel), hipMemcpyDeviceToHost, ctx->stream));
        if (out_pairs && NP) HIP_TRY(hipMemcpyAsync(h_pair, d_pair, cnt * NP * sizeof(impop_dist_pair), hipMemcpyDeviceToHost, ctx->stream));
        if (hist_within && B) HIP_TRY(hipMemcpyAsync(h_hw, d_hw, cnt * K * B * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (hist_between && B && NP) HIP_TRY(hipMemcpyAsync(h_hb, d_hb, cnt * NP * B * 4, hipMemcpyDeviceToHost, ctx->stream));
        return IMPOP_OK;
    }
    void collect(const PairChunk &c) override {
        for (uint64_t k = 0; k < c.cnt; ++k) {
            memcpy(out_panels + c.ord[k] * K, h_pan + k * K, (size_t)K * sizeof(impop_dist_panel));
            if (out_pairs && NP) memcpy(out_pairs + c.ord[k] * NP, h_pair + k * NP, (size_t)NP * sizeof(impop_dist_pair));
            if (hist_within && B) memcpy(hist_within + c.ord[k] * K * B, h_hw + k * K * B, (size_t)K * B * 4);
            if (hist_between && B && NP) memcpy(hist_between + c.ord[k] * NP * B, h_hb + k * NP * B, (size_t)NP * B * 4);
        }
    }
};

// impop_pca_scan's epilogue (pca.hip): one launch of the eigen kernel per chunk — records and vectors; the symmetric distance
// matrices the kernel gathers live in scratch, one per window of a chunk.  With the window distances wanted, every window's
// vectors, eigenvalues and usability also go to tables that live across the chunks, in the caller's window order.
struct PcaEpilogue final : PairEpilogue {
    uint32_t M, k, max_iter;
    double tol;
    bool h16, want_dist;
    uint64_t n_windows;
    const std::vector<uint32_t> *hap_of;
    impop_pca_window *out_windows;
    double *out_vectors;  // nullable
    uint64_t chunks = 0, launches = 0;
    uint32_t *d_hap = nullptr, *d_ok = nullptr;
    char *d_hs = nullptr;
    uint64_t *d_ord = nullptr;
    impop_pca_window *d_rec = nullptr, *h_rec = nullptr;
    double *d_vec = nullptr, *h_vec = nullptr, *d_allvec = nullptr, *d_lam = nullptr, *d_dist = nullptr;
    size_t hs_bytes() const { return (size_t)M * M * (h16 ? 2 : 4); }
    // the device bytes layout() takes per window of a chunk (they bound a chunk: impop_pca_scan)
    size_t per_window_bytes() const { return hs_bytes() + sizeof(impop_pca_window) + (size_t)k * M * 8 + 8; }
    void layout(Layout &D, Layout &H, uint64_t cap) override {
        D.sub(d_hap, M); D.sub(d_ord, cap); D.sub(d_rec, cap); D.sub(d_vec, out_vectors ? cap * k * M : 0);
        D.sub(d_allvec, want_dist ? n_windows * k * M : 0); D.sub(d_lam, want_dist ? n_windows * 8 : 0);
        D.sub(d_ok, want_dist ? n_windows : 0); D.sub(d_dist, want_dist ? n_windows * n_windows : 0);
        D.sub(d_hs, cap * hs_bytes());
        H.sub(h_rec, cap); H.sub(h_vec, out_vectors ? cap * k * M : 0);
    }
    int upload(impop_ctx *ctx) override {
        HIP_TRY(hipMemcpyAsync(d_hap, hap_of->data(), (size_t)M * 4, hipMemcpyHostToDevice, ctx->stream));
        return IMPOP_OK;
    }
    int launch(impop_ctx *ctx, const PairChunk &c) override {
        const uint64_t cnt = c.cnt;
        if (want_dist) HIP_TRY(hipMemcpyAsync(d_ord, c.ord, cnt * 8, hipMemcpyHostToDevice, ctx->stream));
        size_t slot = 0;  // the eigen kernel between two events of its own: impop_ctx_pca_elapsed
        int rc = ctx->gram_timing ? ctx->timers[impop_ctx::T_PCA].begin(ctx->stream, &slot) : IMPOP_OK;
        if (rc) return rc;
        const PcaIn in{d_hap, d_hs, want_dist ? d_ord : nullptr, M, k, max_iter, h16 ? 1u : 0u, tol};
        const PcaOut O{d_rec, out_vectors ? d_vec : nullptr, want_dist ? d_allvec : nullptr, want_dist ? d_lam : nullptr,
                       want_dist ? d_ok : nullptr};  // (a table of zero bytes shares its offset with what follows it)
        rc = launch_pca_eigen(ctx, c.b, cnt, c.d_s, in, O);
        if (rc) return rc;
        if (ctx->gram_timing && (rc = ctx->timers[impop_ctx::T_PCA].end(ctx->stream, slot))) return rc;
        ++chunks; ++launches;
        HIP_TRY(hipMemcpyAsync(h_rec, d_rec, cnt * sizeof(impop_pca_window), hipMemcpyDeviceToHost, ctx->stream));
        if (out_vectors) HIP_TRY(hipMemcpyAsync(h_vec, d_vec, cnt * k * M * 8, hipMemcpyDeviceToHost, ctx->stream));
        return IMPOP_OK;
    }
    void collect(const PairChunk &c) override {
        for (uint64_t i = 0; i < c.cnt; ++i) {
            out_windows[c.ord[i]] = h_rec[i];
            if (out_vectors) memcpy(out_vectors + c.ord[i] * k * M, h_vec + i * k * M, (size_t)k * M * 8);
        }
    }
};

// impop_kinship_scan's epilogue (kinship.hip): per chunk the window kernel (records, watch rows, the diagonals) and, when the
// per-pair totals are wanted, the totals kernel, which adds the chunk's tables into d_tot; d_tot lives across the chunks
struct KinshipEpilogue final : PairEpilogue {
    uint32_t N, n_watch;
    int64_t num, den;
    const uint32_t *watch;            // 2 x n_watch, host
    impop_kin_window *out_windows;
    impop_kin_watch *out_watch;       // nullable
    bool want_totals;
    uint64_t chunks = 0, launches = 0;
    uint32_t *d_watch = nullptr, *d_diag = nullptr;
    uint64_t *d_tot = nullptr, *d_part = nullptr;
    impop_kin_window *d_win = nullptr, *h_win = nullptr;
    impop_kin_watch *d_wat = nullptr, *h_wat = nullptr;
    size_t n_totals() const { return want_totals ? (size_t)N * (N - 1) / 2 * 9 : 0; }
    void layout(Layout &D, Layout &H, uint64_t cap) override {
        D.sub(d_watch, 2 * (size_t)n_watch); D.sub(d_tot, n_totals());
        const uint32_t Z = want_totals ? kinship_total_slices(N, cap) : 1u;  // the most slices a chunk of up to cap windows takes
        D.sub(d_part, Z > 1 ? Z * n_totals() : 0);
        D.sub(d_diag, cap * 2 * N); D.sub(d_win, cap); D.sub(d_wat, cap * n_watch);
        H.sub(h_win, cap); H.sub(h_wat, cap * n_watch);
    }
    int upload(impop_ctx *ctx) override {
        if (n_watch) HIP_TRY(hipMemcpyAsync(d_watch, watch, 2 * (size_t)n_watch * 4, hipMemcpyHostToDevice, ctx->stream));
        if (want_totals) HIP_TRY(hipMemsetAsync(d_tot, 0, n_totals() * 8, ctx->stream));
        return IMPOP_OK;
    }
    int launch(impop_ctx *ctx, const PairChunk &c) override {
        const uint64_t cnt = c.cnt;
        size_t slot = 0;  // the epilogue kernels between two events of their own: impop_ctx_kinship_elapsed
        int rc = ctx->gram_timing ? ctx->timers[impop_ctx::T_KIN + 1].begin(ctx->stream, &slot) : IMPOP_OK;
        if (rc) return rc;
        const KinshipOut O{d_win, n_watch ? d_wat : nullptr, want_totals ? d_tot : nullptr, d_diag, d_part};
        if ((rc = launch_kinship_windows(ctx, c.b, cnt, N, num, den, d_watch, n_watch, O))) return rc;
        ++launches;
        if (want_totals) {
            if ((rc = launch_kinship_totals(ctx, c.b, cnt, N, O))) return rc;
            launches += kinship_total_slices(N, cnt) > 1 ? 2 : 1;
        }
        if (ctx->gram_timing && (rc = ctx->timers[impop_ctx::T_KIN + 1].end(ctx->stream, slot))) return rc;
        ++chunks;
        HIP_TRY(hipMemcpyAsync(h_win, d_win, cnt * sizeof(impop_kin_window), hipMemcpyDeviceToHost, ctx->stream));
        if (n_watch) HIP_TRY(hipMemcpyAsync(h_wat, d_wat, cnt * n_watch * sizeof(impop_kin_watch), hipMemcpyDeviceToHost, ctx->stream));
        return IMPOP_OK;
    }
    void collect(const PairChunk &c) override {
        for (uint64_t k = 0; k < c.cnt; ++k) {
            out_windows[c.ord[k]] = h_win[k];
            if (n_watch) memcpy(out_watch + c.ord[k] * n_watch, h_wat + k * n_watch, (size_t)n_watch * sizeof(impop_kin_watch));
        }
    }
};

// impop_permtest_scan's epilogue (permtest.hip): per chunk the preparation kernel (byte planes of every pair's distance matrix,
// row sums, tie masks, the observed integers) and the labelling kernel (the null integers on the matrix cores, compared and counted on
// the device); the doubles of a record are finalised here, on the host, from the integers (perm_math.h)
struct PermtestEpilogue final : PairEpilogue {
    PermtestTables T{};
    uint32_t n_perm;
    const std::vector<uint32_t> *hap_of, *merged, *moff;
    const std::vector<uint64_t> *z0, *labels, *loff;
    impop_perm_pair *out_pairs;
    impop_perm_null *out_null;  // nullable
    uint64_t chunks = 0, launches = 0;
    uint32_t *d_hap = nullptr, *d_merged = nullptr, *d_moff = nullptr;
    uint64_t *d_z0 = nullptr, *d_labels = nullptr, *d_loff = nullptr;
    PermtestScratch X{};
    PermObs *h_obs = nullptr;
    uint32_t *h_ge = nullptr, *h_st = nullptr;
    uint64_t *h_null = nullptr;
    impop_window_stats *h_ws = nullptr;
    const impop_window_stats *d_ws = nullptr;
    // the device bytes layout() takes per window of a chunk (they bound a chunk: impop_permtest_scan)
    size_t per_window_bytes() const {
        const size_t mp = T.m_pad_max;
        return (size_t)T.NP * (mp * mp * T.planes + mp * T.mw_max * 8 + mp * 16 + sizeof(PermObs) + 16 + (out_null ? (size_t)n_perm * 24 : 0));
    }
    void layout(Layout &D, Layout &H, uint64_t cap) override {
        const size_t slots = cap * T.NP, mp = T.m_pad_max;
        D.sub(d_hap, T.M); D.sub(d_merged, merged->size()); D.sub(d_moff, T.NP + 1);
        D.sub(d_z0, z0->size()); D.sub(d_labels, labels->size()); D.sub(d_loff, T.NP);
        D.sub(X.planes, slots * mp * mp * T.planes); D.sub(X.ties, slots * mp * T.mw_max); D.sub(X.rows, slots * mp);
        D.sub(X.term, slots * mp); D.sub(X.st, slots * mp); D.sub(X.obs, slots); D.sub(X.ge, slots * 4);
        D.sub(X.null, out_null ? slots * n_perm * 3 : 0);
        H.sub(h_obs, slots); H.sub(h_ge, slots * 4); H.sub(h_st, slots * mp); H.sub(h_null, out_null ? slots * n_perm * 3 : 0);
        H.sub(h_ws, cap);
    }
    int upload(impop_ctx *ctx) override {
        HIP_TRY(hipMemcpyAsync(d_hap, hap_of->data(), (size_t)T.M * 4, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(d_merged, merged->data(), merged->size() * 4, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(d_moff, moff->data(), moff->size() * 4, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(d_z0, z0->data(), z0->size() * 8, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(d_labels, labels->data(), labels->size() * 8, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(d_loff, loff->data(), loff->size() * 8, hipMemcpyHostToDevice, ctx->stream));
        T.hap_of = d_hap; T.merged = d_merged; T.moff = d_moff; T.z0 = d_z0; T.labels = d_labels; T.loff = d_loff;
        if (!out_null) X.null = nullptr;  // (a table of zero bytes shares its offset with what follows it)
        return IMPOP_OK;
    }
    int launch(impop_ctx *ctx, const PairChunk &c) override {
        const uint64_t cnt = c.cnt, slots = cnt * T.NP;
        HIP_TRY(hipMemsetAsync(X.ge, 0, slots * 16, ctx->stream));
        size_t s0 = 0, s1 = 0;  // the two kernels between events of their own: impop_ctx_permtest_elapsed
        int rc = ctx->gram_timing ? ctx->timers[impop_ctx::T_PERM].begin(ctx->stream, &s0) : IMPOP_OK;
        if (rc) return rc;
        if ((rc = launch_permtest_prep(ctx, c.b, cnt, T, X))) return rc;
        if (ctx->gram_timing && (rc = ctx->timers[impop_ctx::T_PERM].end(ctx->stream, s0))) return rc;
        if (ctx->gram_timing && (rc = ctx->timers[impop_ctx::T_PERM + 1].begin(ctx->stream, &s1))) return rc;
        if ((rc = launch_permtest_labels(ctx, cnt, T, X))) return rc;
        if (ctx->gram_timing && (rc = ctx->timers[impop_ctx::T_PERM + 1].end(ctx->stream, s1))) return rc;
        ++chunks; launches += 2;
        HIP_TRY(hipMemcpyAsync(h_obs, X.obs, slots * sizeof(PermObs), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(h_ge, X.ge, slots * 16, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(h_st, X.st, slots * T.m_pad_max * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(h_ws, c.d_s, cnt * sizeof(impop_window_stats), hipMemcpyDeviceToHost, ctx->stream));
        if (out_null) HIP_TRY(hipMemcpyAsync(h_null, X.null, slots * n_perm * 24, hipMemcpyDeviceToHost, ctx->stream));
        return IMPOP_OK;
    }
    void collect(const PairChunk &c) override {
        for (uint64_t k = 0; k < c.cnt; ++k)
            for (uint32_t p = 0, a = 0; a < T.K; ++a)
                for (uint32_t b = a + 1; b < T.K; ++b, ++p) {
                    const uint64_t slot = k * T.NP + p;
                    const PermObs &o = h_obs[slot];
                    const uint32_t m_k = T.off[a + 1] - T.off[a], m_l = T.off[b + 1] - T.off[b], *ge = h_ge + slot * 4;
                    const PermDoubles d = perm_doubles(o, m_k, m_l);
                    impop_perm_pair r;
                    r.n_a = m_k; r.n_b = m_l; r.n_sites = h_ws[k].n_sites; r.n_perm = n_perm;
                    r.wa = o.wa; r.wb = o.wb; r.ab = o.tot - o.wa - o.wb; r.nn = o.nn;
                    r.ge_fst = ge[0]; r.ge_phi = ge[1]; r.ge_dxy = ge[2]; r.ge_snn = ge[3];
                    r.fst = d.fst; r.phi_st = d.phi_st; r.dxy = d.dxy; r.snn = perm_snn(h_st + slot * T.m_pad_max, m_k + m_l);
                    r.p_fst = perm_p(ge[0], n_perm); r.p_phi = perm_p(ge[1], n_perm); r.p_dxy = perm_p(ge[2], n_perm);
                    r.p_snn = perm_p(ge[3], n_perm);
                    out_pairs[c.ord[k] * T.NP + p] = r;
                    if (out_null) memcpy(out_null + (c.ord[k] * T.NP + p) * n_perm, h_null + slot * n_perm * 3, (size_t)n_perm * 24);
                }
    }
};

// ---- what the entry points share -------------------------------------------------------------------------------------------
// the checks of impop_pairwise_params common to the calls that take one
int check_pairwise_params(const impop_pairwise_params *params, const char *fn) {
    REQUIRE(params->struct_size == sizeof(impop_pairwise_params), "impop_pairwise_params.struct_size mismatch");
    REQUIRE(params->identity_kind == IMPOP_IDENTITY_MATCH || params->identity_kind == IMPOP_IDENTITY_DICE, "%s: unknown identity kind", fn);
    REQUIRE(params->round_digits <= 19, "%s: round_digits > 19 unsupported", fn);
    REQUIRE(params->d_pi_mode >= 0 && params->d_pi_mode <= 2 && params->s_scope >= 0 && params->s_scope <= 2, "%s: bad d_pi_mode / s_scope", fn);
    return IMPOP_OK;
}
int check_windows(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows, const char *fn) {
    for (uint64_t i = 0; i < n_windows; ++i) {
        const int rc = check_pairwise_args(ctx, m, windows[i].site_begin, windows[i].site_end, fn);
        if (rc) return rc;
    }
    return IMPOP_OK;
}
// the haplotypes a mask selects, ascending (no mask: all n): a view of member_set, whose other two tables are not needed here
std::vector<uint32_t> mask_members(const uint64_t *mask, uint32_t n) { return member_set(mask, n, (n + 31) / 32).idx; }

}  // namespace
static_assert(sizeof(impop_panel_stats) == 48 && sizeof(impop_panel_window) == 8 && sizeof(impop_pair_stats) == 48, "fixed record layouts");

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
    const uint32_t n = m->g.n_hap, K = n_pop, NP = K * (K - 1) / 2, mwords = (n + 63) / 64;
    std::vector<uint8_t> cls(n, 0xFF);
    std::vector<uint32_t> hap_of;  // the panels' members back to back, each ascending: position -> haplotype
    PairdistEpilogue epi;
    uint64_t p_max = 0;
    for (uint32_t k = 0; k < K; ++k) {
        epi.T.off[k] = (uint32_t)hap_of.size();
        for (uint32_t i : mask_members(masks + (size_t)k * mwords, n)) {
            REQUIRE(cls[i] == 0xFF, "%s: populations must be disjoint (population %u overlaps population %u)", fn, k, (uint32_t)cls[i]);
            cls[i] = (uint8_t)k;
            hap_of.push_back(i);
        }
        REQUIRE(hap_of.size() > epi.T.off[k], "%s: population %u is empty", fn, k);
    }
    for (uint32_t k = K; k < 9; ++k) epi.T.off[k] = (uint32_t)hap_of.size();
    if (hap_of.size() > IMPOP_PAIRDIST_MAX_N) {  // refused before anything is uploaded or launched
        set_error("%s: the panels hold %zu members, more than the limit of %u", fn, hap_of.size(), (uint32_t)IMPOP_PAIRDIST_MAX_N);
        return IMPOP_E_UNSUPPORTED;
    }
    const uint32_t M = (uint32_t)hap_of.size();
    if (!n_windows) return IMPOP_OK;
    REQUIRE(windows && out_panels, "%s: NULL windows/out", fn);
    int rc = check_windows(ctx, m, windows, n_windows, fn);
    if (rc) return rc;
    // per pair of panels: both panels' positions merged into ascending haplotype index (the order of the S_nn sum)
    std::vector<uint32_t> merged, moff(1, 0u);
    for (uint32_t a = 0; a < K; ++a) {
        const uint64_t ma = epi.T.off[a + 1] - epi.T.off[a];
        p_max = std::max(p_max, ma * (ma - 1) / 2);
        for (uint32_t b = a + 1; b < K; ++b) {
            p_max = std::max(p_max, ma * (epi.T.off[b + 1] - epi.T.off[b]));
            uint32_t i = epi.T.off[a], j = epi.T.off[b];
            while (i < epi.T.off[a + 1] || j < epi.T.off[b + 1])
                merged.push_back(j >= epi.T.off[b + 1] || (i < epi.T.off[a + 1] && hap_of[i] < hap_of[j]) ? i++ : j++);
            moff.push_back((uint32_t)merged.size());
        }
    }
    const uint64_t max_W = widest_W(m, windows, n_windows);
    if (!pd_sum_h2_admitted(max_W, p_max)) {  // before any launch
        set_error("%s: sum_h2 may overflow 64 bits: the widest window has W = %llu and the largest record %llu pairs (W^2 x pairs must stay "
                  "below 2^64)", fn, (unsigned long long)max_W, (unsigned long long)p_max);
        return IMPOP_E_UNSUPPORTED;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    epi.K = K; epi.NP = NP; epi.M = M; epi.T.K = K; epi.T.M = M;
    epi.B = (hist_within || (hist_between && NP)) ? params->hist_bins : 0u;
    epi.width = params->hist_width;
    epi.hap_of = &hap_of; epi.merged = &merged; epi.moff = &moff;
    epi.out_panels = out_panels; epi.out_pairs = out_pairs; epi.hist_within = hist_within; epi.hist_between = hist_between;
    // histograms in LDS where every counter fits next to the kernel's tables; IMPOP_PAIRDIST_LDS_BINS=n lowers what the LDS form
    // takes, so that tests reach the global form at small sizes
    if (epi.B) {
        const size_t fixed = pairdist_lds_fixed(K, M);
        size_t cap = fixed < PAIRDIST_LDS_BYTES ? (PAIRDIST_LDS_BYTES - fixed) / 4 : 0;
        const char *e = getenv("IMPOP_PAIRDIST_LDS_BINS");
        if (e && *e) {
            const long v = strtol(e, nullptr, 10);
            cap = std::min<size_t>(cap, v < 0 ? 0 : (size_t)v);
        }
        epi.hist_lds = (size_t)(K + NP) * epi.B <= cap;
    }
    PairFront in{};
    in.fn = fn; in.identity_kind = IMPOP_IDENTITY_MATCH; in.round_digits = -1;
    in.scan_host = nullptr; in.use_segmap = false; in.max_W = max_W;
    // the per-member tables and the histograms of a chunk: at most 512 MiB of them
    in.max_chunk_windows = std::min<uint64_t>(65535, std::max<uint64_t>(1, (512ull << 20) / epi.per_window_bytes()));
    rc = pairwise_front(ctx, m, windows, n_windows, in, epi);
    if (rc) return rc;
    if (trace_on())
        fprintf(stderr, "[impop_pairdist_scan] pops=%u pairs=%u members=%u windows=%llu chunks=%llu launches=%llu hist_bins=%u hist=%s\n", K, NP,
                M, (unsigned long long)n_windows, (unsigned long long)epi.chunks, (unsigned long long)epi.launches, epi.B,
                !epi.B ? "off" : epi.hist_lds ? "lds" : "global");
    return IMPOP_OK;
}

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
    const uint32_t n = m->g.n_hap, K = n_pop, NP = K * (K - 1) / 2, mwords = (n + 63) / 64, n_perm = params->n_perm;
    std::vector<uint8_t> cls(n, 0xFF);
    std::vector<uint32_t> hap_of;  // the panels' members back to back, each ascending: position -> haplotype
    PermtestEpilogue epi;
    for (uint32_t k = 0; k < K; ++k) {
        epi.T.off[k] = (uint32_t)hap_of.size();
        for (uint32_t i : mask_members(masks + (size_t)k * mwords, n)) {
            REQUIRE(cls[i] == 0xFF, "%s: populations must be disjoint (population %u overlaps population %u)", fn, k, (uint32_t)cls[i]);
            cls[i] = (uint8_t)k;
            hap_of.push_back(i);
        }
        REQUIRE(hap_of.size() > epi.T.off[k], "%s: population %u is empty", fn, k);
    }
    for (uint32_t k = K; k < 9; ++k) epi.T.off[k] = (uint32_t)hap_of.size();
    if (hap_of.size() > IMPOP_PERMTEST_MAX_N) {  // refused before anything is uploaded or launched
        set_error("%s: the panels hold %zu members, more than the limit of %u", fn, hap_of.size(), (uint32_t)IMPOP_PERMTEST_MAX_N);
        return IMPOP_E_UNSUPPORTED;
    }
    if (out_null && (n_windows > (1ull << 22) || n_windows * NP * n_perm > (1ull << 22))) {
        set_error("%s: a null table of %llu windows x %u pairs x %u labellings exceeds 2^22 entries", fn, (unsigned long long)n_windows, NP, n_perm);
        return IMPOP_E_UNSUPPORTED;
    }
    if (!n_windows) return IMPOP_OK;
    REQUIRE(windows && out_pairs, "%s: NULL windows/out", fn);
    int rc = check_windows(ctx, m, windows, n_windows, fn);
    if (rc) return rc;
    uint64_t p_max = 0;
    for (uint32_t k = 0; k < K; ++k) p_max = std::max<uint64_t>(p_max, perm_q(epi.T.off[k + 1] - epi.T.off[k]));
    const uint64_t max_W = widest_W(m, windows, n_windows);
    if (!perm_fst_admitted(max_W, p_max)) {  // before any launch
        set_error("%s: the Fst comparison may overflow: the widest window has W = %llu and the largest panel %llu pairs (W x pairs^2 must "
                  "stay at or below 2^62)", fn, (unsigned long long)max_W, (unsigned long long)p_max);
        return IMPOP_E_UNSUPPORTED;
    }
    // per pair of panels: both panels' positions merged into ascending haplotype index, the observed labelling over that order, and
    // the labellings themselves (the one generator: perm_math.h perm_labelling)
    std::vector<uint32_t> merged, moff(1, 0u), fy(IMPOP_PERMTEST_MAX_N);
    std::vector<uint64_t> z0, labels, loff;
    uint32_t m_max = 0;
    for (uint32_t a = 0; a < K; ++a)
        for (uint32_t b = a + 1; b < K; ++b) m_max = std::max(m_max, epi.T.off[a + 1] - epi.T.off[a] + epi.T.off[b + 1] - epi.T.off[b]);
    const uint32_t mw_max = (m_max + 63) / 64;
    for (uint32_t a = 0, p = 0; a < K; ++a)
        for (uint32_t b = a + 1; b < K; ++b, ++p) {
            uint32_t i = epi.T.off[a], j = epi.T.off[b];
            z0.resize((size_t)(p + 1) * mw_max, 0ull);
            for (uint32_t at = 0; i < epi.T.off[a + 1] || j < epi.T.off[b + 1]; ++at) {
                const bool from_a = j >= epi.T.off[b + 1] || (i < epi.T.off[a + 1] && hap_of[i] < hap_of[j]);
                if (from_a) z0[(size_t)p * mw_max + (at >> 6)] |= 1ull << (at & 63u);
                merged.push_back(from_a ? i++ : j++);
            }
            moff.push_back((uint32_t)merged.size());
            const uint32_t mp = moff[p + 1] - moff[p], mw = (mp + 63) / 64;
            loff.push_back(labels.size());
            labels.resize(labels.size() + (size_t)n_perm * mw);
            for (uint32_t r = 0; r < n_perm; ++r)
                perm_labelling(params->seed, p, r, mp, epi.T.off[a + 1] - epi.T.off[a], fy.data(), labels.data() + loff[p] + (size_t)r * mw);
        }
    HIP_TRY(hipSetDevice(ctx->device));
    epi.T.K = K; epi.T.M = (uint32_t)hap_of.size(); epi.T.NP = NP; epi.T.n_perm = n_perm;
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
    epi.T.mw_max = mw_max; epi.T.m_pad_max = 64 * mw_max;
    epi.n_perm = n_perm;
    epi.hap_of = &hap_of; epi.merged = &merged; epi.moff = &moff; epi.z0 = &z0; epi.labels = &labels; epi.loff = &loff;
    epi.out_pairs = out_pairs; epi.out_null = out_null;
    PairFront in{};
    in.fn = fn; in.identity_kind = IMPOP_IDENTITY_MATCH; in.round_digits = -1;  // Hamming distances: no unflip pass
    in.scan_host = nullptr; in.use_segmap = false; in.max_W = max_W;
    // the byte planes, tie masks and null rows of a chunk: at most 1 GiB of them
    in.max_chunk_windows = std::min<uint64_t>(65535, std::max<uint64_t>(1, (1ull << 30) / epi.per_window_bytes()));
    rc = pairwise_front(ctx, m, windows, n_windows, in, epi);
    if (rc) return rc;
    if (trace_on())
        fprintf(stderr, "[impop_permtest_scan] route=%s pops=%u pairs=%u members=%u perms=%u planes=%u windows=%llu chunks=%llu launches=%llu "
                "null=%s\n", m->compact ? "compact" : "dense", K, NP, epi.T.M, n_perm, epi.T.planes, (unsigned long long)n_windows,
                (unsigned long long)epi.chunks, (unsigned long long)epi.launches, out_null ? "on" : "off");
    return IMPOP_OK;
}

static_assert(sizeof(impop_pca_params) == 24 && sizeof(impop_pca_window) == 160, "fixed record layouts");
static_assert(IMPOP_PCA_MAX_N == PCA_MAX_N && IMPOP_PCA_MAX_K == PCA_MAX_K && PCA_MAX_K + 8 <= PCA_B, "the block holds k + 8 columns");

IMPOP_API int impop_pca_scan(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows,
                             const uint64_t *mask_p, const impop_pca_params *params, impop_pca_window *out_windows, double *out_vectors,
                             double *out_dist2) {
    const char *fn = "impop_pca_scan";
    REQUIRE(ctx && m && params, "%s: NULL argument", fn);
    REQUIRE(params->struct_size == sizeof(impop_pca_params), "impop_pca_params.struct_size mismatch");
    REQUIRE(params->k >= 1 && params->k <= IMPOP_PCA_MAX_K, "%s: k must be 1..%u", fn, (uint32_t)IMPOP_PCA_MAX_K);
    REQUIRE(params->tol >= 1e-13 && params->tol <= 1e-2, "%s: tol must be in [1e-13, 1e-2]", fn);
    REQUIRE(params->max_iter >= 1 && params->max_iter <= 100000, "%s: max_iter must be 1..100000", fn);
    const std::vector<uint32_t> hap_of = mask_members(mask_p, m->g.n_hap);
    REQUIRE(hap_of.size() >= 2, "%s: the mask holds %zu members, fewer than 2", fn, hap_of.size());
    if (hap_of.size() > IMPOP_PCA_MAX_N) {  // refused before anything is uploaded or launched
        set_error("%s: the mask holds %zu members, more than the limit of %u", fn, hap_of.size(), (uint32_t)IMPOP_PCA_MAX_N);
        return IMPOP_E_UNSUPPORTED;
    }
    if (out_dist2 && n_windows > 16384) {
        set_error("%s: window distances of %llu windows, more than the limit of 16384", fn, (unsigned long long)n_windows);
        return IMPOP_E_UNSUPPORTED;
    }
    REQUIRE(!out_dist2 || out_vectors, "%s: out_dist2 needs out_vectors", fn);
    if (!n_windows) return IMPOP_OK;
    REQUIRE(windows && out_windows, "%s: NULL windows/out", fn);
    int rc = check_windows(ctx, m, windows, n_windows, fn);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const uint64_t max_W = widest_W(m, windows, n_windows);
    PcaEpilogue epi;
    epi.M = (uint32_t)hap_of.size(); epi.k = params->k; epi.max_iter = params->max_iter; epi.tol = params->tol;
    epi.h16 = max_W < 65536;  // a distance is at most its window's W
    epi.want_dist = out_dist2 != nullptr; epi.n_windows = n_windows;
    epi.hap_of = &hap_of; epi.out_windows = out_windows; epi.out_vectors = out_vectors;
    PairFront in{};
    in.fn = fn; in.identity_kind = IMPOP_IDENTITY_MATCH; in.round_digits = -1;  // Hamming distances: no unflip pass
    in.scan_host = nullptr; in.use_segmap = false; in.max_W = max_W;
    // the gathered distance matrices and the vectors of a chunk: at most 1 GiB of them
    in.max_chunk_windows = std::min<uint64_t>(65535, std::max<uint64_t>(1, (1ull << 30) / epi.per_window_bytes()));
    rc = pairwise_front(ctx, m, windows, n_windows, in, epi);
    if (rc) return rc;
    if (out_dist2) {  // the scratch the front end bound the all-window tables into is still the context's
        size_t slot = 0;
        if (ctx->gram_timing && (rc = ctx->timers[impop_ctx::T_PCA + 1].begin(ctx->stream, &slot))) return rc;
        rc = launch_pca_dist(ctx, epi.d_allvec, epi.d_lam, epi.d_ok, epi.M, epi.k, n_windows, epi.d_dist);
        if (rc) return rc;
        if (ctx->gram_timing && (rc = ctx->timers[impop_ctx::T_PCA + 1].end(ctx->stream, slot))) return rc;
        ++epi.launches;
        HIP_TRY(hipMemcpyAsync(out_dist2, epi.d_dist, n_windows * n_windows * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    if (trace_on()) {
        uint32_t it_max = 0;
        uint64_t bad = 0;
        for (uint64_t i = 0; i < n_windows; ++i) {
            it_max = std::max(it_max, out_windows[i].iterations);
            bad += out_windows[i].flags & 1u;
        }
        fprintf(stderr, "[impop_pca_scan] route=%s members=%u k=%u windows=%llu chunks=%llu launches=%llu iterations_max=%u unconverged=%llu "
                "dist=%s\n", m->compact ? "compact" : "dense", epi.M, epi.k, (unsigned long long)n_windows, (unsigned long long)epi.chunks,
                (unsigned long long)epi.launches, it_max, (unsigned long long)bad, out_dist2 ? "on" : "off");
    }
    return IMPOP_OK;
}

static_assert(sizeof(impop_kin_window) == 48 && sizeof(impop_kin_pair) == 72 && sizeof(impop_kin_watch) == 16 &&
                  sizeof(impop_kinship_params) == 16, "fixed record layouts");

IMPOP_API int impop_kinship_scan(impop_ctx *ctx, const impop_genotypes *g, const impop_window *windows, uint64_t n_windows,
                                 const impop_kinship_params *params, const uint32_t *watch, uint32_t n_watch,
                                 impop_kin_window *out_windows, impop_kin_pair *out_pairs, impop_kin_watch *out_watch) {
    const char *fn = "impop_kinship_scan";
    REQUIRE(ctx && g && g->planes && params, "%s: NULL argument", fn);
    REQUIRE(params->struct_size == sizeof(impop_kinship_params), "impop_kinship_params.struct_size mismatch");
    REQUIRE(params->kin_den >= 1 && params->kin_den <= (1u << 20) && params->kin_num <= params->kin_den,
            "%s: the threshold kin_num / kin_den needs 1 <= kin_den <= 2^20 and kin_num <= kin_den", fn);
    const impop_matrix *m = g->planes;
    const uint32_t N = g->n_ind;
    REQUIRE(m->device == ctx->device, "%s: genotypes live on device %d, context on %d", fn, m->device, ctx->device);
    REQUIRE(n_watch <= IMPOP_KINSHIP_MAX_WATCH, "%s: %u watched pairs exceed the limit (%u)", fn, n_watch, (uint32_t)IMPOP_KINSHIP_MAX_WATCH);
    REQUIRE(!n_watch || (watch && out_watch), "%s: NULL watch / out_watch with n_watch = %u", fn, n_watch);
    for (uint32_t q = 0; q < n_watch; ++q) {
        const uint32_t a = watch[2 * q], b = watch[2 * q + 1];
        REQUIRE(a < N && b < N, "%s: watched pair %u: individual %u outside the handle's %u", fn, q, a < N ? b : a, N);
        REQUIRE(a != b, "%s: watched pair %u names individual %u twice", fn, q, a);
    }
    if (!n_windows) return IMPOP_OK;
    REQUIRE(windows && out_windows, "%s: NULL windows/out", fn);
    int rc = check_windows(ctx, m, windows, n_windows, fn);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    KinshipEpilogue epi;
    epi.N = N; epi.n_watch = n_watch; epi.num = params->kin_num; epi.den = params->kin_den;
    epi.watch = watch; epi.out_windows = out_windows; epi.out_watch = out_watch; epi.want_totals = out_pairs != nullptr;
    PairFront in{};
    in.fn = fn; in.identity_kind = IMPOP_IDENTITY_MATCH; in.round_digits = -1;  // no polarity row: the counts are used as written
    in.scan_host = nullptr; in.use_segmap = false; in.max_W = widest_W(m, windows, n_windows);
    rc = pairwise_front(ctx, m, windows, n_windows, in, epi);
    if (rc) return rc;
    if (out_pairs) {  // the scratch the front end bound the totals into is still the context's
        HIP_TRY(hipMemcpyAsync(out_pairs, epi.d_tot, epi.n_totals() * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    if (trace_on())
        fprintf(stderr, "[impop_kinship_scan] route=%s individuals=%u rows=%u windows=%llu chunks=%llu launches=%llu watch=%u plane_bytes=%llu\n",
                m->compact ? "compact" : "dense", N, m->n_hap_pad, (unsigned long long)n_windows, (unsigned long long)epi.chunks,
                (unsigned long long)epi.launches, n_watch, (unsigned long long)m->rb_bytes);
    return IMPOP_OK;
}

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
    std::vector<uint8_t> cls(n, 0xFF);
    std::vector<uint32_t> idx, sizes(K, 0);
    for (uint32_t k = 0; k < K; ++k) {
        for (uint32_t i : mask_members(masks + (size_t)k * mwords, n)) {
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
    if ((rc = check_windows(ctx, m, windows, n_windows, fn))) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
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
    in.scan_host = nullptr; in.use_segmap = use_segmap; in.max_W = widest_W(m, windows, n_windows);
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
    if (!n_windows) return IMPOP_OK;
    REQUIRE(windows && out_host, "%s: NULL windows/out", fn);
    if ((rc = check_windows(ctx, m, windows, n_windows, fn))) return rc;
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
    rc = (want_s && !use_segmap) ? impop_scan_plan_create(ctx, m, windows, n_windows, mask_p, mask_a, mask_b, &sp, &plan) : IMPOP_OK;
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
    epi.idx = &idx; epi.ia = &ia; epi.ib = &ib; epi.fa = &fa; epi.fb = &fb; epi.out_host = out_host;
    PairFront in{};
    in.fn = fn; in.identity_kind = params->identity_kind; in.round_digits = params->round_digits;
    in.scan_host = plan ? scan_host.data() : nullptr; in.use_segmap = use_segmap; in.max_W = widest_W(m, windows, n_windows);
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
    if (!n_windows) return IMPOP_OK;
    REQUIRE(windows && out_host, "impop_cluster_scan: NULL windows/out");
    const int rc = check_windows(ctx, m, windows, n_windows, "impop_cluster_scan");
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    ClusterEpilogue epi;
    epi.params = params; epi.mask_p = mask_p; epi.nP = nP; epi.idx = &idx; epi.out_host = out_host;
    epi.cluster_of = cluster_of; epi.sizes = sizes;
    PairFront in{};
    in.fn = "impop_cluster_scan"; in.identity_kind = params->identity_kind; in.round_digits = params->round_digits;
    in.scan_host = nullptr; in.use_segmap = false;  // the site scan for S / D is not needed (impop_pairwise_scan's s_scope 2)
    in.max_W = widest_W(m, windows, n_windows);
    epi.adj_bytes = af_small_certain(params->identity_kind, nP, m->n_hap_pad, in.max_W) ? 0 : af_adjacency_bytes(nP);
    // the general form keeps a window's adjacency rows in memory (20 MB at the limit): chunks of at most 2 GiB of them
    in.max_chunk_windows = std::min<uint64_t>(65535, std::max<uint64_t>(1, (2ull << 30) / epi.per_window_bytes()));
    return pairwise_front(ctx, m, windows, n_windows, in, epi);
}
