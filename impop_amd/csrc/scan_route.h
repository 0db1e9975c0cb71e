// scan_route.h — the front end the streaming calls share (bodies in scan.hip): which layout a scan of a window list streams
// and how the windows are cut into tiles.  impop_scan_plan_create, impop_scan_multi, impop_haplotype_scan and impop_dstat_scan
// take their route from scan_route; impop_diploid_scan cuts its tiles on the matrix's own rows (tile_cut.h); they and
// impop_ld_scan share the window checks.  The chunked calls among them go on through win_chunks.h (member set, chunk cutter)
// and chunk_run.h (the stream protocol of a chunk).  Below it, the host half of the K-population calls (impop_scan_multi,
// impop_dstat_scan; their device half is pop_stream.h): the panel's masks, its upload, its launch.
#pragma once
#include <type_traits>
#include <vector>

#include "chunk_run.h"
#include "internal.h"
#include "tile_cut.h"

namespace impop {

// What a scan of `windows` streams, derived once per call (scan_route below).
struct ScanRoute : TileCut {  // ... and how cut_tiles cut it: tiles, singles, wins, bytes_streamed
    bool indexed = false;  // the variable-site index (d_vsb, tiles in kept-site coordinates), else d_sb (dense, or a compacted matrix)
    bool split = false;    // ... and its rare-entry stream (d_vrare)
    const uint32_t *sb = nullptr;
    const uint64_t *rare = nullptr;  // null unless split
    // packed: the rare sites come from the matrix's two packed streams instead of d_vrare: rare = d_vmulti, single = d_vsingle.
    // Only scan_route sets it, and only for a caller that asked (impop_scan_plan_create for the fixed-WPS kernel).
    bool packed = false;
    const uint16_t *single = nullptr;
    // unique-row route: the whole 64-row blocks of a tile come from the matrix's distinct-row stream (uniq = d_vuniq, uniq_wt =
    // d_vuniq_wt, uniqs[k] = tile k's range of it) and only the partial blocks at window edges from sb.  Set like packed, for the
    // same caller, whether or not the route is packed.
    const uint32_t *uniq = nullptr;
    const uint8_t *uniq_wt = nullptr;
    bool wave_tiles = false;  // ... and the kernel will run one wave per tile (tile_cut.h, wave_tile_choice)
    // ... from the plan's tile digest (tile_digest.h; only impop_scan_plan_create's plans): bytes_streamed then counts what such a
    // launch reads, digest_rare_streamed of it for histograms, kept singleton ranges and entries
    bool digest = false;
    uint64_t digest_rare_streamed = 0;
    std::vector<LayoutWindow> lw;  // the windows as ranges of sb's sites, of rare's entries (split) and of single's (packed)
    uint32_t tile_blocks = 0;
};

// the windows as ranges of the rows of m->d_sb (a compacted matrix: original coordinates -> kept-site index ranges)
std::vector<LayoutWindow> row_windows(const impop_matrix *m, const impop_window *windows, uint64_t n_windows);
// every window lies in the matrix and is at most 2^32 - 1 sites long
int check_windows(const char *fn, const impop_matrix *m, const impop_window *windows, uint64_t n_windows);
// every window's W (window_W: its length, or the sum of its columns' weights) fits the 32 bits a record gives it
int check_window_weights(const char *fn, const impop_matrix *m, const impop_window *windows, uint64_t n_windows);
// windows (validated, matrix coordinates) -> the route of a scan of m and what a launch on it streams.  tile_blocks 0: the default.
// want_packed: the caller's kernel reads the singleton stream and the distinct-row stream; the route is packed when the matrix
// has the one and a unique-row route when it has the other (else as without).  trace: print the route's trace line (a caller
// that goes on deciding what the line reports passes false and calls trace_route itself, once)
int scan_route(const char *fn, impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows,
               uint32_t tile_blocks, ScanRoute &rt, bool want_packed = false, bool trace = true);
void trace_route(const impop_matrix *m, const ScanRoute &rt, uint64_t n_windows);
// a tile-size override for tests, <name>=n in the environment: n clamped to 1..4096, 0 where the variable is unset or empty
uint32_t env_tile_blocks(const char *name);

// K populations as the kernels of pop_stream.h read them
struct PopPanel {
    std::vector<uint32_t> mk;  // K x wps dwords, clipped to n_hap
    std::vector<uint32_t> nk;  // K sizes
};
// masks: K bitsets of ceil(n_hap / 64) words.  Refuses nothing: which populations must be disjoint or non-empty is each call's own rule.
void pop_panel_pack(const impop_matrix *m, const uint64_t *masks, uint32_t K, PopPanel &p);

struct PopPanelDev {
    ScanTile *tiles = nullptr;
    WinDesc *wins = nullptr;
    uint32_t *masks = nullptr, *n = nullptr;
};
// Lists the route's tiles and windows and the panel's masks and sizes in L, then what own(L) adds (the call's partials and
// records), gets L.total() bytes of the context's scratch, binds every listed pointer and queues the four uploads on the
// context's stream.
int pop_panel_upload(impop_ctx *ctx, const ScanRoute &rt, const PopPanel &p, PopPanelDev &dev, const std::function<void(Layout &)> &own);

// One streaming launch of a kernel of pop_stream.h: a workgroup per tile, the K masks in dynamic LDS (above 48 KiB by opt-in).
// Every such kernel starts with (sb, rare, tiles, masks, pop_n, wps, G, r, weights); own... is what follows.
template <typename Kernel, typename... Own>
int pop_launch(Kernel kernel, uint32_t K, hipStream_t st, const impop_matrix *m, const ScanRoute &rt, const PopPanelDev &dev,
               const uint32_t *weights, Own... own) {
    const size_t lds = (size_t)K * ((m->g.wps + 3) & ~3u) * 4;
    const int rc = lds_opt_in(kernel, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(kernel, dim3((uint32_t)rt.tiles.size()), dim3(256), lds, st, rt.sb, rt.rare, (const ScanTile *)dev.tiles,
                       (const uint32_t *)dev.masks, (const uint32_t *)dev.n, m->g.wps, m->g.G, m->g.r, weights, own...);
    HIP_TRY(hipGetLastError());
    return IMPOP_OK;
}
// f(std::integral_constant<int, k>()) for the run-time k in KMIN..8 (validated by the caller)
template <int KMIN, typename F>
int pop_dispatch_k(uint32_t k, F f) {
    if constexpr (KMIN < 8) {
        if (k > (uint32_t)KMIN) return pop_dispatch_k<KMIN + 1>(k, f);
    }
    return f(std::integral_constant<int, KMIN>());
}

}  // namespace impop
