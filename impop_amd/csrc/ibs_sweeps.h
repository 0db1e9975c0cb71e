// ibs_sweeps.h — the count and fill sweeps of ibs.hip as an internal call: impop_ibs_scan is one caller, impop_ibd_scan (ibd.hip)
// the other.  A client keeps the tracts on the device: after the counting sweep every range of pairs whose tracts fit the staging
// is filled and handed over, pair-major and ascending, and the client runs its own pass over them before the next range.
#pragma once
#include <functional>

#include "internal.h"

namespace impop {

struct IbsStage {                  // the staged tracts of the pairs [p0, p1)
    uint64_t p0, p1, n_pairs;
    const impop_ibs_pair *d_rec;   // the records of all pairs (h1, h2, n_tracts)
    const uint64_t *d_off;         // n_pairs + 1 offsets into the call's whole tract list
    const impop_ibs_segment *d_seg;  // tract d_off[p] - off0 + k is the k-th of pair p
    uint64_t off0, cnt;            // d_off[p0], and the tracts staged
};

struct IbsClient {
    int timer = 0;                 // first of the three timer slots the sweeps use
    size_t extra_bytes = 0;        // device memory of the client's own that lives as long as the call
    std::function<int(void *d_extra, uint64_t n_pairs)> prepare;  // before the first launch: uploads into d_extra
    std::function<int(const IbsStage &)> range;                   // per pair range, tracts or none; leaves the stream synchronised
    uint64_t n_pairs = 0, tracts = 0, pair_ranges = 0, launches = 0, bytes_streamed = 0;  // out
};

int ibs_scan_run(const char *fn, impop_ctx *ctx, const impop_matrix *m, const uint64_t *mask_p, const uint32_t *pairs, uint64_t n_pairs,
                 const impop_window *windows, uint64_t n_windows, uint64_t b, uint64_t e, uint32_t min_sites, uint64_t max_chunk_bytes,
                 impop_ibs_pair *pair_out, impop_ibs_segment *seg_out, uint64_t seg_capacity, uint64_t *n_segments,
                 impop_ibs_window *win_out, IbsClient *client);

}  // namespace impop
