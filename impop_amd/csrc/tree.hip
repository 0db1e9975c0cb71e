// tree.hip — impop_tree_scan: its kernel, its PairEpilogue (pair_front.h) and the entry point.  Per window the exact single /
// complete / average (UPGMA) linkage tree of the members of one mask over their Hamming distances, in integers with a fixed tie
// rule (all arithmetic: tree_math.h), and per panel the largest clade inside it and its most recent common ancestor.
//
// One workgroup per window, of 256 threads up to 256 members, 512 up to 512, 1024 beyond, so that a thread owns one row.  The
// workgroup first gathers the symmetric m x m matrix into its slice of the epilogue's scratch from the Gram kernel's upper triangle
// (as pca.hip does; uint32 where every sum the linkage can form fits, else uint64), then runs the m - 1 merges.  Nobody rescans the
// matrix per step: LDS keeps per live row its nearest neighbour and that entry.  A step is
//   1. the argmin over the rows' cached neighbours, with the number of rows that attain the minimum value (one reduction: a
//      butterfly inside a wave, the waves' results through LDS);
//   2. Lance-Williams on row and column a from row b (one entry per thread, rows a and b read coalesced), each row k comparing
//      its new entry (k, a) with its cached one; rows whose cached neighbour was a or b, and row a, go to a list;
//   3. sizes, liveness, the panels' counts (thread p < K owns panel p);
//   4. the listed rows rescanned from the matrix, a wave per row, coalesced.
// Four barriers per step.
#include "pair_front.h"
#include "tree_math.h"

namespace impop {

constexpr uint32_t TREE_ROW_BATCH = 8;  // loads a lane issues before it compares (tree_scan_row)

struct TreeIn {
    const uint32_t *hap_of;  // m: haplotype index of a position
    const uint8_t *cls;      // m: the panel of a position, 0xFF = none (K > 0)
    void *ss;                // scratch: n_problems x m x m sums, symmetric, ST
    uint32_t m, K, linkage;
    uint32_t psize[TREE_MAX_POP];
};
struct TreeOut {
    impop_tree_window *rec;   // n_problems
    impop_tree_merge *merges;  // n_problems x (m - 1), or nullptr
    impop_tree_panel *panels;  // n_problems x K (K > 0)
    uint32_t *recomputed;      // n_problems: rows the merges invalidated (the trace line)
};

struct TreeLds {
    uint64_t *val, *sh;
    TreeBest *red;  // [2][16 waves]: two buffers in turn, so that one barrier per reduction is enough
    uint32_t *size, *nn, *list, *hap, *diag, *ctl;
    uint16_t *cnt;  // K x m: members of panel p in the cluster named k
};
static size_t tree_lds_bytes(uint32_t m, uint32_t K) {
    return (size_t)m * 8 + 16 * 8 + 2 * 16 * sizeof(TreeBest) + (size_t)m * 4 * 5 + 16 + (size_t)K * m * 2;
}
__device__ __forceinline__ TreeLds tree_carve(uint64_t *base, uint32_t m) {
    TreeLds L;
    L.val = base; L.sh = L.val + m;
    L.red = reinterpret_cast<TreeBest *>(L.sh + 16);
    L.size = reinterpret_cast<uint32_t *>(L.red + 32);
    L.nn = L.size + m; L.list = L.nn + m; L.hap = L.list + m; L.diag = L.hap + m; L.ctl = L.diag + m;
    L.cnt = reinterpret_cast<uint16_t *>(L.ctl + 4);
    return L;
}

__device__ __forceinline__ TreeKey tree_shfl_key(const TreeKey &k, int off) {
    TreeKey r;
    r.num = __shfl_xor(k.num, off, 64);
    r.den = __shfl_xor(k.den, off, 64);
    const uint32_t ab = __shfl_xor((k.a << 16) | (k.b & 0xFFFFu), off, 64);  // names < 1024; TREE_NONE comes back as 0xFFFF
    r.a = ab >> 16; r.b = ab & 0xFFFFu;
    if (r.a == 0xFFFFu) r.a = r.b = TREE_NONE;
    return r;
}

// the nearest neighbour of the live row k under the order of tree_math.h: lanes stride the row, then a butterfly (all lanes get it)
template <typename ST>
__device__ __forceinline__ TreeKey tree_scan_row(const ST *row, uint32_t k, uint32_t m, const uint32_t *size, uint32_t linkage, uint32_t lane) {
    TreeKey best = tree_key_none();
    const uint32_t sk = size[k];
    // eight loads in flight per lane before the first comparison: a row of 512 members is one round trip, not eight
    for (uint32_t j0 = lane; j0 < m; j0 += 64 * TREE_ROW_BATCH) {
        ST x[TREE_ROW_BATCH];
#pragma unroll
        for (uint32_t u = 0; u < TREE_ROW_BATCH; ++u) x[u] = j0 + 64 * u < m ? row[j0 + 64 * u] : (ST)0;
#pragma unroll
        for (uint32_t u = 0; u < TREE_ROW_BATCH; ++u) {
            const uint32_t j = j0 + 64 * u;
            const uint32_t sj = j < m ? size[j] : 0u;
            if (j == k || !sj) continue;
            const TreeKey key = tree_key(linkage, (uint64_t)x[u], sk, sj, k, j);
            if (tree_key_less(key, best)) best = key;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const TreeKey other = tree_shfl_key(best, off);
        if (tree_key_less(other, best)) best = other;
    }
    return best;
}

template <typename ST, int NT>
__global__ __launch_bounds__(NT) void tree_kernel(SimBatch batch, const impop_window_stats *__restrict__ ws, TreeIn in, TreeOut out) {
    extern __shared__ uint64_t tree_smem[];
    constexpr uint32_t NW = NT / 64;
    const uint32_t m = in.m, K = in.K, linkage = in.linkage, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t w = blockIdx.x;
    const TreeLds L = tree_carve(tree_smem, m);
    const SimView S = sim_view(batch, w);
    const bool no_sites = S.W == 0;  // every H is 0

    // ---- gather: H symmetric into scratch, from the Gram upper triangle (members ascend, so (p, q > p) is (min, max)); sum_h
    for (uint32_t p = tid; p < m; p += NT) {
        const uint32_t h = in.hap_of[p];
        L.hap[p] = h;
        L.diag[p] = no_sites ? 0u : (uint32_t)gram_at(S, h, h);
        L.size[p] = 1u;
        for (uint32_t c = 0; c < K; ++c) L.cnt[(size_t)c * m + p] = in.cls[p] == c ? 1u : 0u;
    }
    if (tid == 0) L.ctl[0] = 0;
    __syncthreads();
    ST *Ss = reinterpret_cast<ST *>(in.ss) + w * (uint64_t)m * m;
    uint64_t part = 0;
    for (uint32_t p = wave; p < m; p += NW) {
        const uint32_t hp = L.hap[p], ap = L.diag[p];
        for (uint32_t q = p + lane; q < m; q += 64) {
            uint32_t H = 0;
            if (q != p && !no_sites) H = ap + L.diag[q] - 2u * (uint32_t)gram_at(S, hp, L.hap[q]);
            Ss[(uint64_t)p * m + q] = (ST)H;
            Ss[(uint64_t)q * m + p] = (ST)H;
            part += H;
        }
    }
    const uint64_t sum_h = block_sum_u64_n<NT>(part, L.sh);
    __threadfence_block();  // the matrix was written by other waves of this workgroup
    __syncthreads();

    // ---- every row's nearest neighbour
    for (uint32_t k = wave; k < m; k += NW) {
        const TreeKey key = tree_scan_row(Ss + (uint64_t)k * m, k, m, L.size, linkage, lane);
        if (lane == 0) { L.nn[k] = key.a == k ? key.b : key.a; L.val[k] = key.num; }
    }
    __syncthreads();

    uint32_t n_zero = 0, n_tied = 0, recomputed = 0;  // thread 0's
    TreeMerge last{0u, 0u, 0u, 0u, 0ull};
    TreePanel P = tree_panel_start(tid < K ? in.psize[tid] : 1u);  // thread p < K's
    impop_tree_merge *mg = out.merges ? out.merges + w * (uint64_t)(m - 1) : nullptr;
    int buf = 0;
    for (uint32_t step = 0; step + 1 < m; ++step) {
        // ---- 1. the pair to merge
        TreeBest mine = tree_best_none();
        uint32_t my_nn = TREE_NONE, my_size = 0;
        uint64_t my_val = 0;
        if (tid < m && (my_size = L.size[tid]) != 0) {
            my_nn = L.nn[tid]; my_val = L.val[tid];
            mine = tree_best_of_row(tree_key(linkage, my_val, my_size, L.size[my_nn], tid, my_nn));
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            TreeBest other;
            other.key = tree_shfl_key(mine.key, off);
            other.rows = __shfl_xor(mine.rows, off, 64);
            mine = tree_best_combine(mine, other);
        }
        buf ^= 1;
        if (lane == 0) L.red[buf * 16 + wave] = mine;
        if (tid == 0) L.ctl[0] = 0;  // the list is empty: its readers finished before the last barrier, its writers start behind the next
        __syncthreads();
        TreeBest best = L.red[buf * 16];
#pragma unroll
        for (uint32_t v = 1; v < NW; ++v) best = tree_best_combine(best, L.red[buf * 16 + v]);
        const uint32_t a = best.key.a, b = best.key.b, sa = L.size[a], sb = L.size[b];
        // ---- 2. row and column a from row b; the caches
        if (tid < m && my_size && tid != a && tid != b) {
            const uint64_t x = tree_lance_williams(linkage, (uint64_t)Ss[(uint64_t)a * m + tid], (uint64_t)Ss[(uint64_t)b * m + tid]);
            Ss[(uint64_t)a * m + tid] = (ST)x;
            Ss[(uint64_t)tid * m + a] = (ST)x;
            if (!tree_cache_survives(my_nn, a, b)) L.list[atomicAdd(&L.ctl[0], 1u)] = tid;
            else if (tree_key_less(tree_key(linkage, x, my_size, sa + sb, tid, a),
                                   tree_key(linkage, my_val, my_size, L.size[my_nn], tid, my_nn))) {
                L.nn[tid] = a;
                L.val[tid] = x;
            }
        }
        if (tid == a) L.list[atomicAdd(&L.ctl[0], 1u)] = a;
        if (tid == 0) {
            last = TreeMerge{a, b, sa, sb, best.key.num};
            if (mg) { mg[step].a = a; mg[step].b = b; mg[step].size_a = sa; mg[step].size_b = sb; mg[step].num = best.key.num; }
            tree_count_merge(best.key.num, best.rows, n_zero, n_tied);
        }
        __threadfence_block();
        __syncthreads();
        // ---- 3. sizes, liveness, panels
        if (tid == a) L.size[a] = sa + sb;
        if (tid == b) L.size[b] = 0u;
        if (tid < K) L.cnt[(size_t)tid * m + a] = (uint16_t)tree_panel_merge(P, L.cnt[(size_t)tid * m + a], L.cnt[(size_t)tid * m + b], sa + sb, step);
        __syncthreads();
        // ---- 4. the rows the merge invalidated (row b, which pointed at a, retires)
        const uint32_t n_list = L.ctl[0];
        if (tid == 0) recomputed += n_list + 1u;
        if (step + 2 < m)
            for (uint32_t i = wave; i < n_list; i += NW) {
                const uint32_t k = L.list[i];
                const TreeKey key = tree_scan_row(Ss + (uint64_t)k * m, k, m, L.size, linkage, lane);
                if (lane == 0) { L.nn[k] = key.a == k ? key.b : key.a; L.val[k] = key.num; }
            }
        __syncthreads();
    }
    if (tid < K) {
        impop_tree_panel *pr = out.panels + w * K + tid;
        pr->n_members = P.n_members; pr->largest_clade = P.largest_clade; pr->mrca_size = P.mrca_size; pr->mrca_merge = P.mrca_merge;
    }
    if (tid == 0) {
        impop_tree_window *rec = out.rec + w;
        rec->n_members = m; rec->n_sites = ws[w].n_sites; rec->n_zero_merges = n_zero; rec->n_tied_merges = n_tied; rec->sum_h = sum_h;
        rec->root_num = last.num; rec->root_size_a = last.size_a; rec->root_size_b = last.size_b; rec->reserved = 0;
        out.recomputed[w] = recomputed;
    }
}

template <typename ST, int NT>
static int launch_tree_as(impop_ctx *ctx, const SimBatch &b, uint64_t n, const impop_window_stats *d_stats, const TreeIn &in, const TreeOut &out,
                          size_t lds) {
    const int rc = lds_opt_in(tree_kernel<ST, NT>, lds);
    if (rc) return rc;
    hipLaunchKernelGGL((tree_kernel<ST, NT>), dim3((uint32_t)n), dim3(NT), lds, ctx->stream, b, d_stats, in, out);
    return IMPOP_OK;
}

static int launch_tree(impop_ctx *ctx, const SimBatch &b, uint64_t n_problems, const impop_window_stats *d_stats, const TreeIn &in,
                       const TreeOut &out, bool wide) {
    if (!n_problems) return IMPOP_OK;
    REQUIRE(in.m >= 2 && in.m <= TREE_MAX_N && in.K <= TREE_MAX_POP && in.linkage <= TREE_AVERAGE, "launch_tree: bad shape");
    const size_t lds = tree_lds_bytes(in.m, in.K);
    REQUIRE(lds <= 160 * 1024, "launch_tree: %zu bytes of LDS", lds);
    int rc;
    if (!wide) rc = in.m <= 256 ? launch_tree_as<uint32_t, 256>(ctx, b, n_problems, d_stats, in, out, lds)
                  : in.m <= 512 ? launch_tree_as<uint32_t, 512>(ctx, b, n_problems, d_stats, in, out, lds)
                                : launch_tree_as<uint32_t, 1024>(ctx, b, n_problems, d_stats, in, out, lds);
    else rc = in.m <= 256 ? launch_tree_as<uint64_t, 256>(ctx, b, n_problems, d_stats, in, out, lds)
            : in.m <= 512 ? launch_tree_as<uint64_t, 512>(ctx, b, n_problems, d_stats, in, out, lds)
                          : launch_tree_as<uint64_t, 1024>(ctx, b, n_problems, d_stats, in, out, lds);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return IMPOP_OK;
}

// impop_tree_scan's epilogue: one launch of the tree kernel per chunk — records, merges, panels; the matrices the kernel gathers
// and rewrites live in scratch, one per window of a chunk.
struct TreeEpilogue final : PairEpilogue {
    uint32_t M, K, linkage;
    bool wide;  // the sums are stored as uint64
    uint32_t psize[TREE_MAX_POP];
    const std::vector<uint32_t> *hap_of;
    const std::vector<uint8_t> *cls;
    Result<impop_tree_window> rec;
    Result<impop_tree_merge> merges;
    Result<impop_tree_panel> panels;
    Result<uint32_t> recomputed;  // consumed here: never scattered
    uint64_t launches = 0, rows_recomputed = 0;
    uint32_t *d_hap = nullptr;
    uint8_t *d_cls = nullptr;
    char *d_ss = nullptr;
    size_t ss_bytes() const { return (size_t)M * M * (wide ? 8 : 4); }
    // the device bytes layout() takes per window of a chunk (they bound a chunk: impop_tree_scan)
    size_t per_window_bytes() const {
        return ss_bytes() + sizeof(impop_tree_window) + (size_t)(M - 1) * sizeof(impop_tree_merge) + (size_t)K * sizeof(impop_tree_panel) + 4;
    }
    void layout(Layout &D, Layout &H, uint64_t cap) override {
        D.sub(d_hap, M); D.sub(d_cls, M);
        rec.layout(D, H, cap); merges.layout(D, H, cap); panels.layout(D, H, cap); recomputed.layout(D, H, cap);
        D.sub(d_ss, cap * ss_bytes());
    }
    int upload(impop_ctx *ctx) override {
        HIP_TRY(hipMemcpyAsync(d_hap, hap_of->data(), (size_t)M * 4, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(d_cls, cls->data(), (size_t)M, hipMemcpyHostToDevice, ctx->stream));
        return IMPOP_OK;
    }
    int launch(impop_ctx *ctx, const PairChunk &c) override {
        TreeIn in{d_hap, d_cls, d_ss, M, K, linkage, {}};
        memcpy(in.psize, psize, sizeof psize);
        const TreeOut O{rec.d, merges.n ? merges.d : nullptr, panels.d, recomputed.d};
        // the tree kernel between two events of its own: impop_ctx_tree_elapsed
        int rc = timed(ctx, ctx->timers[impop_ctx::T_TREE], [&] { return launch_tree(ctx, c.b, c.cnt, c.d_s, in, O, wide); });
        if (rc) return rc;
        ++launches;
        if ((rc = rec.down(ctx, c.cnt))) return rc;
        if ((rc = merges.down(ctx, c.cnt))) return rc;
        if ((rc = panels.down(ctx, c.cnt))) return rc;
        return recomputed.down(ctx, c.cnt);
    }
    void collect(const PairChunk &c) override {
        rec.scatter(c); merges.scatter(c); panels.scatter(c);
        for (uint64_t k = 0; k < c.cnt; ++k) rows_recomputed += recomputed.h[k];
    }
};

}  // namespace impop

using namespace impop;

static_assert(sizeof(impop_tree_params) == 8 && sizeof(impop_tree_window) == 48 && sizeof(impop_tree_merge) == 24 &&
              sizeof(impop_tree_panel) == 16, "fixed record layouts");
static_assert(sizeof(TreeMerge) == sizeof(impop_tree_merge) && sizeof(TreePanel) == sizeof(impop_tree_panel), "tree_math.h's records");
static_assert(IMPOP_TREE_MAX_N == TREE_MAX_N && TREE_MAX_POP == PANEL_MAX_K && IMPOP_LINKAGE_SINGLE == TREE_SINGLE &&
              IMPOP_LINKAGE_COMPLETE == TREE_COMPLETE && IMPOP_LINKAGE_AVERAGE == TREE_AVERAGE, "the header's constants");

IMPOP_API int impop_tree_scan(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows,
                              const uint64_t *mask_p, const uint64_t *panel_masks, uint32_t n_pop, const impop_tree_params *params,
                              impop_tree_window *out_windows, impop_tree_merge *out_merges, impop_tree_panel *out_panels) {
    const char *fn = "impop_tree_scan";
    static const char *const names[3] = {"single", "complete", "average"};
    REQUIRE(ctx && m && params, "%s: NULL argument", fn);
    REQUIRE(params->struct_size == sizeof(impop_tree_params), "impop_tree_params.struct_size mismatch");
    REQUIRE(params->linkage <= IMPOP_LINKAGE_AVERAGE, "%s: linkage must be 0 (single), 1 (complete) or 2 (average)", fn);
    REQUIRE(n_pop <= PANEL_MAX_K, "%s: n_pop must be 0..%u", fn, PANEL_MAX_K);
    REQUIRE((n_pop > 0) == (out_panels != nullptr), "%s: out_panels must be given exactly when n_pop > 0", fn);
    REQUIRE(!n_pop || panel_masks, "%s: panel_masks is NULL with n_pop > 0", fn);
    const std::vector<uint32_t> hap_of = mask_members(mask_p, m->g.n_hap);
    REQUIRE(hap_of.size() >= 2, "%s: the mask holds %zu members, fewer than 2", fn, hap_of.size());
    if (hap_of.size() > IMPOP_TREE_MAX_N) {  // refused before anything is uploaded or launched
        set_error("%s: the mask holds %zu members, more than the limit of %u", fn, hap_of.size(), (uint32_t)IMPOP_TREE_MAX_N);
        return IMPOP_E_UNSUPPORTED;
    }
    TreeEpilogue epi;
    epi.M = (uint32_t)hap_of.size(); epi.K = n_pop; epi.linkage = params->linkage;
    std::vector<uint8_t> cls(epi.M, 0xFF);
    memset(epi.psize, 0, sizeof epi.psize);
    if (n_pop) {
        PanelSet ps;
        int rc = panel_refused(panel_set(panel_masks, n_pop, m->g.n_hap, ps), fn);
        if (rc) return rc;
        uint32_t in_mask = 0;
        for (uint32_t p = 0; p < epi.M; ++p) {
            cls[p] = ps.cls[hap_of[p]];
            in_mask += cls[p] != 0xFF;
        }
        REQUIRE(in_mask == ps.M, "%s: %u panel members lie outside mask_p", fn, ps.M - in_mask);
        for (uint32_t k = 0; k < n_pop; ++k) epi.psize[k] = ps.sizes[k];
    }
    bool go;
    int rc = windows_ready(ctx, m, windows, n_windows, out_windows, fn, &go);
    if (rc || !go) return rc;
    const uint64_t max_W = widest_W(m, windows, n_windows);
    // an entry is at most W (single, complete) or W |A| |B| <= W floor(m^2 / 4) (average); IMPOP_TREE_WIDE=1 (a test aid) stores
    // 64-bit sums whatever the bound says
    static const bool wide_env = env_is("IMPOP_TREE_WIDE", '1');
    const uint64_t pairs_max = epi.linkage == IMPOP_LINKAGE_AVERAGE ? (uint64_t)epi.M * epi.M / 4 : 1;
    epi.wide = wide_env || max_W > 0xFFFFFFFFull / pairs_max;
    epi.hap_of = &hap_of; epi.cls = &cls;
    epi.rec.want(out_windows, 1); epi.merges.want(out_merges, epi.M - 1); epi.panels.want(out_panels, n_pop);
    epi.recomputed.n = 1;
    // the matrices and the merge lists of a chunk: at most 1 GiB of them
    PairFront in = hamming_front(fn, max_W, chunk_windows(1ull << 30, epi.per_window_bytes()));
    rc = pairwise_front(ctx, m, windows, n_windows, in, epi);
    if (rc) return rc;
    if (trace_on()) {
        uint64_t tied = 0;
        for (uint64_t i = 0; i < n_windows; ++i) tied += out_windows[i].n_tied_merges != 0;
        fprintf(stderr, "[impop_tree_scan] route=%s linkage=%s members=%u pops=%u windows=%llu chunks=%llu launches=%llu rows_recomputed=%llu "
                "tied_windows=%llu\n", m->compact ? "compact" : "dense", names[epi.linkage], epi.M, n_pop, (unsigned long long)n_windows,
                (unsigned long long)in.chunks, (unsigned long long)epi.launches, (unsigned long long)epi.rows_recomputed, (unsigned long long)tied);
    }
    return IMPOP_OK;
}
