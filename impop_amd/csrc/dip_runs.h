// dip_runs.h — the run-length summary of impop_diploid_scan and its associative combine (plain C++, no HIP types:
// tests/fuzz/dip_runs.cc compiles it on the host; diploid.hip runs the same code on the device).
//
// A summary describes one individual's heterozygous sites inside a stretch of sites (a block, a wave's blocks, a tile, a window):
// how many, the coordinates of the first and the last, and the INNER runs — the homozygous stretches between two heterozygous
// sites of the summary.  What lies left of `first` and right of `last` is open: it is closed by the neighbouring summary
// (dip_combine: the gap first_right - last_left - 1 becomes an inner run) or by the window's edges (dip_close).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DIP_HD __host__ __device__
#else
#define DIP_HD
#endif

namespace impop {

struct DipSummary {        // 40 bytes
    uint32_t het;          // heterozygous sites; 0: first / last are meaningless
    uint32_t hom_alt;      // sites where both copies carry the allele
    uint64_t first, last;  // coordinates of the first and the last heterozygous site
    uint32_t longest;      // longest inner run
    uint32_t roh_runs;     // inner runs of at least min_run sites
    uint32_t roh_sites;    // sites inside those
    uint32_t run_sum;      // sites inside all inner runs (the window kernel's consistency check)
};

DIP_HD inline DipSummary dip_empty() { return DipSummary{0u, 0u, 0ull, 0ull, 0u, 0u, 0u, 0u}; }

// a run of `len` sites closed: runs of length 0 are not runs
DIP_HD inline void dip_add_run(DipSummary &s, uint64_t len, uint32_t min_run) {
    const uint32_t l = (uint32_t)len;  // a window is at most 2^32 - 1 sites long
    if (l > s.longest) s.longest = l;
    if (l >= min_run) {  // min_run >= 1
        s.roh_runs += 1;
        s.roh_sites += l;
    }
    s.run_sum += l;
}

// one more heterozygous site at coordinate p, right of everything s holds
DIP_HD inline void dip_append_site(DipSummary &s, uint64_t p, uint32_t min_run) {
    if (s.het == 0) s.first = p;
    else dip_add_run(s, p - s.last - 1, min_run);
    s.last = p;
    s.het += 1;
}

// a (left) joined with b (right): associative, dip_empty() is neutral on both sides
DIP_HD inline DipSummary dip_combine(const DipSummary &a, const DipSummary &b, uint32_t min_run) {
    if (b.het == 0) {
        DipSummary r = a;
        r.hom_alt += b.hom_alt;
        return r;
    }
    if (a.het == 0) {
        DipSummary r = b;
        r.hom_alt += a.hom_alt;
        return r;
    }
    DipSummary r;
    r.het = a.het + b.het;
    r.hom_alt = a.hom_alt + b.hom_alt;
    r.first = a.first;
    r.last = b.last;
    r.longest = a.longest > b.longest ? a.longest : b.longest;
    r.roh_runs = a.roh_runs + b.roh_runs;
    r.roh_sites = a.roh_sites + b.roh_sites;
    r.run_sum = a.run_sum + b.run_sum;
    dip_add_run(r, b.first - a.last - 1, min_run);
    return r;
}

// the summary of window [b, e) closed by the window's edges: the leading run first - b and the trailing run e - 1 - last
// (no heterozygous site: one run of e - b sites).  Afterwards run_sum + het == e - b.
DIP_HD inline DipSummary dip_close(DipSummary s, uint64_t b, uint64_t e, uint32_t min_run) {
    if (s.het == 0) {
        dip_add_run(s, e - b, min_run);
    } else {
        dip_add_run(s, s.first - b, min_run);
        dip_add_run(s, e - 1 - s.last, min_run);
    }
    return s;
}

}  // namespace impop
