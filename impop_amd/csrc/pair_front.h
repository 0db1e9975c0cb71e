// pair_front.h — what the windowed all-pairs calls share: the front end (pairwise_scan.hip) and the PairEpilogue a call hands to it, the
// mover of an epilogue's results, the entry points' common steps, the device view of a panel_set.h set.  A call lives next to its kernels.
#pragma once
#include <string.h>

#include <algorithm>
#include <vector>

#include "chunk_run.h"
#include "panel_set.h"
#include "stats_kernels.h"

namespace impop {

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
    uint64_t chunks;                      // out: the chunks the front end launched
};
int pairwise_front(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows, PairFront &in,
                   PairEpilogue &epi);

// One result of an epilogue: n elements per window in a device sub-buffer d, their page-locked copy h, the caller's array out.  n = 0:
// nothing comes down (want(): an array the caller did not pass).  A result the host consumes itself has no `out`: it is never scattered.
template <typename T>
struct Result {
    T *out = nullptr, *d = nullptr, *h = nullptr;
    size_t n = 0;
    void want(T *out_, size_t per_window) { out = out_; n = out_ ? per_window : 0; }
    // dev_n: the elements per window on the device, where the kernels write the buffer whether or not the result was asked for
    void layout(Layout &D, Layout &H, uint64_t cap, size_t dev_n) { D.sub(d, cap * dev_n); H.sub(h, cap * n); }
    void layout(Layout &D, Layout &H, uint64_t cap) { layout(D, H, cap, n); }
    int down(impop_ctx *ctx, uint64_t cnt) const {
        if (n) HIP_TRY(hipMemcpyAsync(h, d, cnt * n * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
        return IMPOP_OK;
    }
    void scatter(const PairChunk &c) const {  // problem k is window ord[k] of the caller's array
        if (!out || !n) return;
        for (uint64_t k = 0; k < c.cnt; ++k) memcpy(out + c.ord[k] * n, h + k * n, n * sizeof(T));
    }
};

// ---- what the entry points share (bodies in pairwise_scan.hip)
// bounds every Gram count of a call (a cell is a window or a piece of one; compacted: + its constant)
uint64_t widest_W(const impop_matrix *m, const impop_window *windows, uint64_t n_windows);
int check_windows(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows, const char *fn);
// behind a call's own refusals: no windows, nothing to do (*go false); else arrays there, windows the Gram path takes, device current
int windows_ready(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows, const void *out, const char *fn,
                  bool *go);
// the haplotypes a mask selects, ascending (no mask: all n): a view of member_set, whose other two tables are not needed here
inline std::vector<uint32_t> mask_members(const uint64_t *mask, uint32_t n) { return member_set(mask, n, (n + 31) / 32).idx; }
int panel_refused(const PanelRefusal &r, const char *fn);  // IMPOP_OK, or the refusal in the calls' words
// the front end's parameters of a call that takes no scan records (use_segmap: the caller's to set)
inline PairFront front_params(const char *fn, int identity_kind, int round_digits, uint64_t max_W, uint64_t max_chunk_windows = 0) {
    PairFront in{};
    in.fn = fn; in.identity_kind = identity_kind; in.round_digits = round_digits; in.max_W = max_W; in.max_chunk_windows = max_chunk_windows;
    return in;
}
// ... of a call on Hamming distances: `match` (no unflip pass), unrounded, no site bitmap
inline PairFront hamming_front(const char *fn, uint64_t max_W, uint64_t max_chunk_windows = 0) {
    return front_params(fn, IMPOP_IDENTITY_MATCH, -1, max_W, max_chunk_windows);
}
// windows per chunk of an epilogue that takes per_window_bytes of device memory for each: what fits the budget, 1 .. 65535
inline uint64_t chunk_windows(uint64_t budget_bytes, uint64_t per_window_bytes) {
    return std::min<uint64_t>(65535, std::max<uint64_t>(1, budget_bytes / per_window_bytes));
}

// ---- the panels of a panel_set.h PanelSet as the kernels see them
struct PanelTables {
    const uint32_t *hap_of;  // M: haplotype index of a position
    const uint32_t *merged;  // per pair of panels p: the positions of both panels in ascending haplotype index, at moff[p]
    const uint32_t *moff;    // K (K - 1) / 2 + 1
    uint32_t off[9];
    uint32_t K, M;
};
// the three tables in an epilogue's device region, and their upload
struct PanelUpload {
    const PanelSet *set = nullptr;
    const MergedPairs *pairs = nullptr;
    uint32_t *d_hap = nullptr, *d_merged = nullptr, *d_moff = nullptr;
    void layout(Layout &D) {
        D.sub(d_hap, set->M); D.sub(d_merged, pairs->merged.size() ? pairs->merged.size() : 1); D.sub(d_moff, pairs->moff.size());
    }
    int upload(impop_ctx *ctx, PanelTables &T) const {
        HIP_TRY(hipMemcpyAsync(d_hap, set->hap_of.data(), (size_t)set->M * 4, hipMemcpyHostToDevice, ctx->stream));
        if (!pairs->merged.empty()) HIP_TRY(hipMemcpyAsync(d_merged, pairs->merged.data(), pairs->merged.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(d_moff, pairs->moff.data(), pairs->moff.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        T.hap_of = d_hap; T.merged = d_merged; T.moff = d_moff; T.K = set->K; T.M = set->M;
        memcpy(T.off, set->off, sizeof T.off);
        return IMPOP_OK;
    }
};
// pair p of the K (K - 1) / 2 = panels (ka, kb), ka < kb, and its merged list (scalars, not the struct: the callers' loops keep their code)
struct PanelPair {
    uint32_t ka, kb, len;
    const uint32_t *list;
};
__device__ __forceinline__ PanelPair panel_pair(uint32_t K, const uint32_t *merged, const uint32_t *moff, uint32_t p) {
    PanelPair P;
    uint32_t ka = 0, rest = p;
    while (rest >= K - 1 - ka) { rest -= K - 1 - ka; ++ka; }
    P.ka = ka; P.kb = ka + 1 + rest;
    P.list = merged + moff[p];
    P.len = moff[p + 1] - moff[p];
    return P;
}

}  // namespace impop
