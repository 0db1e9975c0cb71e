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
// Unique-row route: a tile's range of the distinct-row stream (internal.h, d_vuniq), in rows of that stream.  A tile's common
// rows [cb, ce) are a head (the part before the first 64-row boundary, if cb % 64 != 0), the whole blocks [g0, g1) between, and a
// tail (the part after the last boundary, if ce % 64 != 0).  The whole blocks are streamed as their representatives with a
// weight each, {ubase[g0], ubase[g1]} of the stream (ubase: the representatives before each block of common rows), where that
// is fewer bytes (uniq_range_of); head and tail as the rows themselves.  A parallel array to the tiles like SingleRange; empty: every row of the tile is streamed as it is.
struct UniqRange {
    uint64_t begin, end;
};
#ifdef __HIPCC__
#define IMPOP_TILE_HD __host__ __device__
#else
#define IMPOP_TILE_HD
#endif
// the whole 64-row blocks [g0, g1) of the rows [cb, ce); g0 >= g1: none
struct MidBlocks {
    uint64_t g0, g1;
    IMPOP_TILE_HD bool any() const { return g1 > g0; }
};
IMPOP_TILE_HD inline MidBlocks mid_blocks(uint64_t cb, uint64_t ce) { return {(cb + 63) / 64, ce > cb ? ce / 64 : 0}; }
// The fixed-WPS kernel's 32-bit lane sums with weights: a representative stands for up to 64 rows, each adding at most 2^16 to a
// sum (c (n - c) and the A x B cross term at n <= 512), so 2^22 per weighted row.  A tile takes the stream only while its whole
// blocks number at most UNIQ_MID_MAX: their representatives then touch at most UNIQ_MID_MAX + 1 blocks of the stream, a lane (one
// wave in four, one row per block) at most ceil(2041 / 4) = 511 of them, 511 x 2^22 < 2^31; the lane's own head or tail row (2^16)
// and its rare sites (2^24, scan.hip single_range) keep the total below 2^32.  A larger tile streams its rows as they are.
constexpr uint64_t UNIQ_MID_MAX = 2040;
constexpr uint64_t UNIQ_ROW_SUM_MAX = 1ull << 16, UNIQ_WEIGHT_MAX = 64, UNIQ_RARE_SUM_MAX = 1ull << 24;
// the largest sum one lane of a 256-thread workgroup can reach for a tile with `mid` whole blocks that takes the stream
inline uint64_t uniq_lane_sum_bound(uint64_t mid) {
    return ((mid + 1 + 3) / 4) * UNIQ_WEIGHT_MAX * UNIQ_ROW_SUM_MAX + UNIQ_ROW_SUM_MAX + UNIQ_RARE_SUM_MAX;
}
// One wave per tile (scan.hip, scan_tiles_kernel_wave): the tile's sums sit in 64 lanes, not 256.  A lane then takes one row of
// EVERY block the tile reads — a representative adds at most UNIQ_WEIGHT_MAX x UNIQ_ROW_SUM_MAX = 2^22, a row of a head, of a tail
// or of a tile without the stream 2^16, counted here as a representative all the same — and one in 64 of the tile's rare words:
// 8-byte entries of the rare stream (one site of minor count m <= 3) and 8-byte words of the singleton stream (four sites of
// m = 1).  A rare site adds m (n - m) <= 3 x 511 or mA (nB - mB) + mB (nA - mA) <= 3 x 512 to a sum, below WAVE_RARE_SITE_SUM_MAX,
// so a word at most four times that.  The entries and the singleton words are two loops of stride 64, each rounded up.
constexpr uint64_t WAVE_RARE_SITE_SUM_MAX = 1ull << 11, WAVE_RARE_WORD_SUM_MAX = 4 * WAVE_RARE_SITE_SUM_MAX;
// the largest sum one lane of a one-wave tile can reach: `blocks` blocks read (rows and representatives), `rare_words` rare words
inline uint64_t wave_lane_sum_bound(uint64_t blocks, uint64_t rare_words) {
    return blocks * UNIQ_WEIGHT_MAX * UNIQ_ROW_SUM_MAX + (rare_words / 64 + 2) * WAVE_RARE_WORD_SUM_MAX;
}
// What a one-wave tile may hold: round figures under wave_lane_sum_bound(...) < 2^32 — 512 x 2^22 = 2^31 for the rows and
// (2^12 + 2) x 2^13 < 2^26 for the rare words.  Far above what one wave is good for (wave_tile_rule): the cap is what makes the
// 32-bit lane sums right, the rule what makes the kernel worth taking.
constexpr uint64_t WAVE_BLOCKS_MAX = 512, WAVE_RARE_WORDS_MAX = 1ull << 18;
static_assert(WAVE_BLOCKS_MAX * UNIQ_WEIGHT_MAX * UNIQ_ROW_SUM_MAX + (WAVE_RARE_WORDS_MAX / 64 + 2) * WAVE_RARE_WORD_SUM_MAX < (1ull << 32),
              "a one-wave tile at the cap overflows a 32-bit lane sum");
inline bool wave_tile_fits(uint64_t blocks, uint64_t rare_words) { return blocks <= WAVE_BLOCKS_MAX && rare_words <= WAVE_RARE_WORDS_MAX; }
// The default choice between the two bodies of the fixed-WPS kernel on a unique-row route, from the plan's number of tiles and
// its largest tile (blocks read; rare words).  One wave per tile pays the per-tile fixed cost — decode, range dispatch, table
// share, reduction, store — once where four waves pay it four times, and takes a quarter of the workgroups; it is the better
// body where tiles are small and many.  False: above the cap (then whatever the override says, the caller runs four waves);
// with fewer than WAVE_RULE_TILES_PER_CU n_cu tiles, where four-wave workgroups reach more CUs and SIMDs than n_tiles / 4 one-wave
// ones do; and with a tile beyond WAVE_RULE_BLOCKS blocks or WAVE_RULE_RARE_WORDS rare words, which one wave walks four times as
// serially as four.  The thresholds are measured on an MI355X at 465 haplotypes (tools/sweep_wave_tiles.py; DESIGN.md 4.1, round
// 25): from 2 048 tiles of 7 to 20 KB one wave wins by more than the four-wave arm's spread and at 1 536 it does not; at 3 072
// and 4 854 tiles it wins up to 100 kb windows as one tile (29 KB: at most 6 blocks read and about 1 200 rare words) and is level
// from 150 kb (38 KB: 7 blocks, 1 800 rare words).  n_cu <= 0 counts as 256, as in default_tile_rule.
constexpr uint64_t WAVE_RULE_TILES_PER_CU = 8, WAVE_RULE_BLOCKS = 6, WAVE_RULE_RARE_WORDS = 1536;
inline bool wave_tile_rule(uint64_t n_tiles, uint64_t max_blocks, uint64_t max_rare_words, int n_cu) {
    if (!wave_tile_fits(max_blocks, max_rare_words)) return false;
    if (n_tiles < WAVE_RULE_TILES_PER_CU * (uint64_t)(n_cu > 0 ? n_cu : 256)) return false;
    return max_blocks <= WAVE_RULE_BLOCKS && max_rare_words <= WAVE_RULE_RARE_WORDS;
}
// override: -1 none (the rule), 0 never, 1 whenever the cap allows (IMPOP_SCAN_WAVE_TILES, read where a plan is made)
inline bool wave_tile_choice(int override_, uint64_t n_tiles, uint64_t max_blocks, uint64_t max_rare_words, int n_cu) {
    if (override_ == 0 || !wave_tile_fits(max_blocks, max_rare_words)) return false;
    return override_ == 1 ? true : wave_tile_rule(n_tiles, max_blocks, max_rare_words, n_cu);
}
// bytes of the blocks of the stream the rows [begin, end) of it touch, whole, each with its 64 weight bytes
IMPOP_TILE_HD inline uint64_t uniq_bytes_streamed(uint64_t begin, uint64_t end, uint32_t wps) {
    return end > begin ? ((end + 63) / 64 - begin / 64) * (256ull * wps + 64ull) : 0;
}
// A tile takes the stream for its whole blocks only where that reads fewer bytes than the blocks themselves (one whole block
// never does: its representatives fill a block of the stream at least, and their weights come on top).
IMPOP_TILE_HD inline UniqRange uniq_range_of(uint64_t cb, uint64_t ce, const uint64_t *ubase, uint32_t wps) {
    const MidBlocks m = mid_blocks(cb, ce);
    if (!m.any() || m.g1 - m.g0 > UNIQ_MID_MAX) return {0, 0};
    const UniqRange u{ubase[m.g0], ubase[m.g1]};
    return uniq_bytes_streamed(u.begin, u.end, wps) < (m.g1 - m.g0) * 256ull * wps ? u : UniqRange{0, 0};
}
// what a workgroup reads of a tile's rows on that route.  u empty: its blocks of rows, whole, as tile_bytes_streamed counts them.
// Else the head's and the tail's block, whole, and the blocks of the stream the range touches, whole, each with its 64 weight bytes.
inline uint64_t tile_row_bytes_streamed(const ScanTile &t, const UniqRange &u, uint32_t wps) {
    if (t.site_end <= t.site_begin) return 0;
    if (u.end <= u.begin) return ((t.site_end + 63) / 64 - t.site_begin / 64) * 256ull * wps;
    const uint64_t edge = (t.site_begin % 64 != 0) + (t.site_end % 64 != 0);
    return edge * 256ull * wps + uniq_bytes_streamed(u.begin, u.end, wps);
}
// the same in blocks, of rows and of the stream alike, and the tile's rare words (entries and singleton words): what
// wave_tile_fits and wave_tile_rule ask of a plan's largest tile
inline uint64_t tile_blocks_read(const ScanTile &t, const UniqRange &u) {
    if (t.site_end <= t.site_begin) return 0;
    if (u.end <= u.begin) return (t.site_end + 63) / 64 - t.site_begin / 64;
    return (t.site_begin % 64 != 0) + (t.site_end % 64 != 0) + ((u.end + 63) / 64 - u.begin / 64);
}
inline uint64_t tile_rare_words(const ScanTile &t, const SingleRange &s) {
    return (t.rare_end - t.rare_begin) + single_bytes_streamed(s) / 8;
}
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
    std::vector<UniqRange> uniqs;      // unique-row route only: uniqs[k] is tile k's range of the distinct-row stream
    std::vector<WinDesc> wins;
    uint64_t bytes_streamed = 0;
    // unique-row route: the tiles are cut (cut_tiles) and every tile's range is known (uniqs, one per tile): count the rows as
    // that route reads them.  Returns the row bytes of the route.
    uint64_t apply_uniq_ranges(uint32_t wps) {
        uint64_t rows = 0;
        for (size_t k = 0; k < tiles.size(); ++k) {
            const ScanTile row_only{tiles[k].site_begin, tiles[k].site_end, 0, 0};
            bytes_streamed -= tile_bytes_streamed(row_only, wps);
            rows += tile_row_bytes_streamed(tiles[k], uniqs[k], wps);
        }
        bytes_streamed += rows;
        return rows;
    }
};

// windows -> elementary segments between sorted window boundaries (a segment is tiled iff some window covers it, and exactly
// once however many windows overlap it) -> tiles of <= tile_blocks 64-site blocks; every window becomes a contiguous tile range
// [t0, t1).  A segment's blocks and rare sites are cut into the same number of tiles by their bytes (a rare site counts 8 B
// whichever stream holds it, tile_blocks blocks the budget): one workgroup reads a share of every stream.  Without rare sites
// the tiles are those of the unsplit index.  Packed: a segment's rare sites are cut where the split route cuts them, and a
// part's share of them is multis and singletons in the segment's own proportion; so the tiles, their number, every window's
// tile range and every tile's count of rare sites are those of the split route.  ubase (unique-row route; the representatives
// before each 64-row block of the sites' layout, one entry past the last whole block): the same tiles, and every tile's range of
// the distinct-row stream (uniq_range_of) with its rows counted as that route reads them.
inline void cut_tiles(const std::vector<LayoutWindow> &windows, uint32_t tile_blocks, uint32_t wps, bool packed, TileCut &out,
                      const uint64_t *ubase = nullptr) {
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
    if (ubase) {
        for (const ScanTile &t : tiles) out.uniqs.push_back(uniq_range_of(t.site_begin, t.site_end, ubase, wps));
        out.apply_uniq_ranges(wps);
    }
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
