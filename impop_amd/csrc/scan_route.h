// scan_route.h — the front end the streaming calls share (bodies in scan.hip): which layout a scan of a window list streams
// and how the windows are cut into tiles.  impop_scan_plan_create, impop_scan_multi and impop_haplotype_scan all go through it.
#pragma once
#include <vector>

#include "internal.h"

namespace impop {

// site_begin..site_end: sites of the SB64 layout streamed; rare_begin..rare_end: entries of the split index's rare stream
// (internal.h, d_vrare).  Either range may be empty.
struct ScanTile {
    uint64_t site_begin, site_end;
    uint64_t rare_begin, rare_end;
};
struct WinDesc {
    uint64_t t0, t1;  // tile range
    uint64_t n_sites;
    uint64_t seq_len;
};

// What a scan of `windows` streams, derived once per call (scan_route below).
struct ScanRoute {
    bool indexed = false;  // the variable-site index (d_vsb, tiles in kept-site coordinates), else d_sb (dense, or a compacted matrix)
    bool split = false;    // ... and its rare-entry stream (d_vrare)
    const uint32_t *sb = nullptr;
    const uint64_t *rare = nullptr;           // null unless split
    std::vector<impop_window> mapped, rare_w;  // the windows as ranges of sb's sites and (split) of rare's entries
    uint32_t tile_blocks = 0;
    std::vector<ScanTile> tiles;
    std::vector<WinDesc> wins;
    uint64_t bytes_streamed = 0;
};

// windows -> elementary segments -> tiles of <= rt.tile_blocks 64-site blocks; every window becomes a contiguous tile range
void build_tiles(ScanRoute &rt, uint64_t n_windows, uint32_t wps);
// every window lies in the matrix and is at most 2^32 - 1 sites long
int check_windows(const char *fn, const impop_matrix *m, const impop_window *windows, uint64_t n_windows);
// windows (validated, matrix coordinates) -> the route of a scan of m and what a launch on it streams.  tile_blocks 0: the default.
int scan_route(const char *fn, impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows,
               uint32_t tile_blocks, ScanRoute &rt);

}  // namespace impop
