// tile_cut.h — how the streaming calls cut a window list into tiles: which bytes every workgroup reads.  Plain C++, no HIP:
// tests/fuzz/tile_cut.cc compiles it on the host under the sanitizers and checks every cut against a brute-force model.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace impop {

// site_begin..site_end: sites of the SB64 layout streamed; rare_begin..rare_end: entries of the split index's rare stream
// (internal.h, d_vrare).  Either range may be empty.
struct ScanTile {
    uint64_t site_begin, site_end;
    uint64_t rare_begin, rare_end;
};
// what a workgroup reads of a tile: its 64-site blocks of 4 wps bytes per site, whole, and its 8-byte rare entries
inline uint64_t tile_bytes_streamed(const ScanTile &t, uint32_t wps) {
    return (t.site_end > t.site_begin ? ((t.site_end + 63) / 64 - t.site_begin / 64) * 256ull * wps : 0) + (t.rare_end - t.rare_begin) * 8ull;
}
// Packed route: a tile's range of the singleton stream (internal.h, d_vsingle), in uint16 units; the tile's rare range is then
// one of d_vmulti.  A parallel array to the tiles, so that ScanTile and the kernels that read only it stay what they are.
struct SingleRange {
    uint64_t begin, end;
};
// what a workgroup reads of it: the aligned 8-byte words (four singletons each) the range touches
inline uint64_t single_bytes_streamed(const SingleRange &r) { return r.end > r.begin ? ((r.end + 3) / 4 - r.begin / 4) * 8ull : 0; }
struct WinDesc {
    uint64_t t0, t1;  // tile range
    uint64_t n_sites;
    uint64_t seq_len;
};

// A window edge in layout coordinates: c = site of the SB64 layout streamed, r = entry of the rare stream, g = singleton.  All
// three map monotonically from the matrix coordinate, so the triples are ordered as the edges are (no rare site between two
// edges means neither a singleton nor a multi between them).  A route without a split has r = g = 0, one without the packed
// streams g = 0.
struct EdgeCut {
    uint64_t c, r, g;
    bool operator<(const EdgeCut &o) const { return c < o.c || (c == o.c && (r < o.r || (r == o.r && g < o.g))); }
    bool operator==(const EdgeCut &o) const { return c == o.c && r == o.r && g == o.g; }
};
struct LayoutWindow {
    EdgeCut lo, hi;
    uint64_t seq_len;
    bool empty() const { return lo == hi; }  // in every stream: lo <= hi in each coordinate
};

struct TileCut {
    std::vector<ScanTile> tiles;
    std::vector<SingleRange> singles;  // packed only: singles[k] is tile k's singleton range
    std::vector<WinDesc> wins;
    uint64_t bytes_streamed = 0;
};

// windows -> elementary segments between sorted window boundaries (a segment is tiled iff some window covers it, and exactly
// once however many windows overlap it) -> tiles of <= tile_blocks 64-site blocks; every window becomes a contiguous tile range
// [t0, t1).  A segment's blocks and rare sites are cut into the same number of tiles by their bytes (a rare site counts 8 B
// whichever stream holds it, tile_blocks blocks the budget): one workgroup reads a share of every stream.  Without rare sites
// the tiles are those of the unsplit index.  Packed: a segment's rare sites are cut where the split route cuts them, and a
// part's share of them is multis and singletons in the segment's own proportion; so the tiles, their number, every window's
// tile range and every tile's count of rare sites are those of the split route.
inline void cut_tiles(const std::vector<LayoutWindow> &windows, uint32_t tile_blocks, uint32_t wps, bool packed, TileCut &out) {
    std::vector<ScanTile> &tiles = out.tiles;
    std::vector<EdgeCut> cuts;
    cuts.reserve(2 * windows.size());
    for (const LayoutWindow &w : windows)
        if (!w.empty()) {
            cuts.push_back(w.lo);
            cuts.push_back(w.hi);
        }
    std::sort(cuts.begin(), cuts.end());
    cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
    std::vector<int64_t> cover(cuts.size() + 1, 0);
    auto cut_index = [&](const EdgeCut &x) { return (size_t)(std::lower_bound(cuts.begin(), cuts.end(), x) - cuts.begin()); };
    for (const LayoutWindow &w : windows)
        if (!w.empty()) {
            cover[cut_index(w.lo)] += 1;
            cover[cut_index(w.hi)] -= 1;
        }
    const uint64_t row_bytes = 64ull * wps * 4ull, budget = (uint64_t)tile_blocks * row_bytes;
    std::vector<uint64_t> seg_tile_start(cuts.size() + 1, 0);
    int64_t depth = 0;
    for (size_t k = 0; k + 1 < cuts.size(); ++k) {
        seg_tile_start[k] = tiles.size();
        depth += cover[k];
        if (depth <= 0) continue;
        // tiles are cut on 64-site block boundaries of the layout so interior tiles read whole blocks, in equal shares:
        // a 781-block segment under a 512-block limit becomes 391 + 390 blocks, not 512 + 269
        const EdgeCut s = cuts[k], e = cuts[k + 1];
        const uint64_t nm = e.r - s.r, nr = nm + (e.g - s.g);  // entries of the rare stream; rare sites, singletons included
        const uint64_t nblk = e.c > s.c ? (e.c + 63) / 64 - s.c / 64 : 0;
        const uint64_t n_parts = std::max<uint64_t>(1, (nblk * row_bytes + nr * 8 + budget - 1) / budget);
        const uint64_t per = (nblk + n_parts - 1) / n_parts, per_r = (nr + n_parts - 1) / n_parts;
        // the first `off` of the segment's nr rare sites hold this many of its nm multis, and singletons for the rest: a part
        // holds exactly the rare sites the split route gives it, at most per_r <= budget / 8
        auto multis = [&](uint64_t off) { return nr ? (uint64_t)((unsigned __int128)nm * off / nr) : 0; };
        uint64_t cs = s.c, rs = 0;
        for (uint64_t part = 0; part < n_parts; ++part) {
            uint64_t ce = cs;
            if (cs < e.c) ce = std::min(e.c, ((cs / 64) + per) * 64);  // block-aligned end
            const uint64_t re = std::min(nr, rs + per_r);
            if (ce > cs || re > rs) {
                tiles.push_back({cs, ce, s.r + multis(rs), s.r + multis(re)});
                out.bytes_streamed += tile_bytes_streamed(tiles.back(), wps);
                if (packed) {
                    out.singles.push_back({s.g + rs - multis(rs), s.g + re - multis(re)});
                    out.bytes_streamed += single_bytes_streamed(out.singles.back());
                }
            }
            cs = ce;
            rs = re;
        }
    }
    if (!cuts.empty()) seg_tile_start[cuts.size() - 1] = tiles.size();
    seg_tile_start[cuts.size()] = tiles.size();
    out.wins.resize(windows.size());
    for (size_t i = 0; i < windows.size(); ++i) {
        const LayoutWindow &w = windows[i];
        out.wins[i] = {w.empty() ? 0 : seg_tile_start[cut_index(w.lo)], w.empty() ? 0 : seg_tile_start[cut_index(w.hi)], w.hi.c - w.lo.c,
                       w.seq_len};
    }
}

// Default tile: ~256 KB of matrix per workgroup (wide sites — the any-n kernel, wps > 16 — go down to 4 blocks = one per
// wave), but never so large that a small job leaves CUs without work (>= 16 tiles per CU wanted), and never below the 32
// blocks the kernel was tuned with.  With few haplotypes a 32-block tile is only a few KB and the per-workgroup costs
// (launch, LDS reduction, partial store) bound the kernel instead of HBM: n = 32 ran at 2.6 TB/s with 32-block tiles and
// 5.0 TB/s with whole-window tiles.  blocks: the 64-site blocks the windows cover, as the caller counts them.
inline uint32_t default_tile_rule(uint32_t wps, uint64_t blocks, int n_cu) {
    const uint32_t by_bytes = wps > 16 ? std::max<uint32_t>(4, 1024 / wps) : std::max<uint32_t>(32, 1024 / wps);
    const uint64_t by_parallelism = blocks / (16ull * (uint64_t)(n_cu > 0 ? n_cu : 256));
    return (uint32_t)std::max<uint64_t>(std::min<uint32_t>(32, by_bytes), std::min<uint64_t>(by_bytes, by_parallelism));
}

}  // namespace impop
