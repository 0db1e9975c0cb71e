// tile_digest.h — the per-plan tile digest of the one-wave body (scan.hip, scan_tiles_kernel_digest): what a tile may hold,
// when a plan takes the digest, and where every tile's share of it lies.  Plain C++, no HIP: tests/fuzz/tile_digest.cc compiles
// it on the host under the sanitizers.
//
// A plan is a matrix and a window list, both immutable for its life; only the three masks change from launch to launch.  So
// everything a tile's sums need that does not depend on the masks is worked out once, where the plan is made:
//   rows        the tile's common rows — head and tail rows of the layout, its whole blocks as their representatives of the
//               distinct-row stream or as rows — grouped once more under complement over the WHOLE tile: the distinct patterns
//               (canonical: haplotype 0 carries 0, padding bits zero) in order of first occurrence, each with a uint16 weight, the
//               number of the tile's rows it stands for.  Every sum and segregating test is linear in that weight.
//   singletons  a singleton site adds to a tile's sums only through its carrier's membership of A, B and P: one uint16 count per
//               haplotype, 32 wps of them, replaces the tile's range of the singleton stream where that range is no shorter.
// Entries of minor count 2 and 3 stay in the rare stream.
#pragma once
#include "tile_cut.h"

namespace impop {

// What a launch reads of tile k on a digest plan (scalar loads of the wave that owns it): its representatives are rows
// [row_off, row_off + n_rows) of the digest (row_off a multiple of DIGEST_ROW_GRAIN), its singletons histogram hist - 1 (hist = 0:
// none, then [single_begin, single_end) of the singleton stream, empty where the tile has no singleton), its entries
// [rare_begin, rare_end) of the rare stream.
struct DigestDesc {  // 48 B
    uint64_t row_off;
    uint32_t n_rows, hist;
    uint64_t rare_begin, rare_end;
    uint64_t single_begin, single_end;
};

// A tile's candidate rows, the rows the build compares: head + representatives + tail where it has a range of the distinct-row
// stream, else every row.
inline uint64_t digest_candidates(const ScanTile &t, const UniqRange &u) {
    if (t.site_end <= t.site_begin) return 0;
    if (u.end <= u.begin) return t.site_end - t.site_begin;
    const MidBlocks m = mid_blocks(t.site_begin, t.site_end);
    return ((m.g0 << 6) - t.site_begin) + (u.end - u.begin) + (t.site_end - (m.g1 << 6));
}

// Exactness.  The build holds a tile's candidates in LDS (DIGEST_ROWS_MAX x 64 B), a weight and a count are 16 bits wide, and the
// eight 32-bit sums of a lane must hold a tile.  A lane takes one representative of every block of 64; a representative of
// weight w adds at most w x UNIQ_ROW_SUM_MAX (w < 2^16 and the product <= 2^16: a 24-bit multiply whose result stays below 2^32),
// and the weights of a tile add up to its common rows, so its rows add at most common_rows x 2^16 to ONE lane, however they are
// grouped.  A singleton adds at most DIGEST_SINGLE_SUM_MAX = 512 (k_X (n_X - 1), or n_B k_A + n_A k_B - 2 k_AB, at n <= 512), and the
// histogram may put every one of them into one lane; a kept range adds what wave_lane_sum_bound counts for its words.  Entries as there.
constexpr uint64_t DIGEST_ROWS_MAX = 512, DIGEST_COMMON_MAX = DIGEST_ROWS_MAX * UNIQ_WEIGHT_MAX, DIGEST_SINGLES_MAX = 65535;
constexpr uint64_t DIGEST_SINGLE_SUM_MAX = 512;
inline uint64_t digest_lane_sum_bound(uint64_t common_rows, uint64_t singles, uint64_t entries) {
    return common_rows * UNIQ_ROW_SUM_MAX + singles * DIGEST_SINGLE_SUM_MAX + (((singles + 3) / 4 + 1) / 64 + 2) * WAVE_RARE_WORD_SUM_MAX +
           (entries / 64 + 2) * WAVE_RARE_SITE_SUM_MAX;
}
static_assert(DIGEST_COMMON_MAX * UNIQ_ROW_SUM_MAX + DIGEST_SINGLES_MAX * DIGEST_SINGLE_SUM_MAX +
                      (((DIGEST_SINGLES_MAX + 3) / 4 + 1) / 64 + 2) * WAVE_RARE_WORD_SUM_MAX +
                      (WAVE_RARE_WORDS_MAX / 64 + 2) * WAVE_RARE_SITE_SUM_MAX < (1ull << 32),
              "a digest tile at the cap overflows a 32-bit lane sum");
static_assert(DIGEST_COMMON_MAX <= 65535 && DIGEST_SINGLES_MAX <= 65535, "a weight or a count overflows 16 bits");
inline bool digest_tile_fits(uint64_t candidates, uint64_t common_rows, uint64_t singles, uint64_t entries) {
    return candidates <= DIGEST_ROWS_MAX && common_rows <= DIGEST_COMMON_MAX && singles <= DIGEST_SINGLES_MAX && entries <= WAVE_RARE_WORDS_MAX;
}
inline bool digest_tile_fits(const ScanTile &t, const UniqRange &u, const SingleRange &s) {
    return digest_tile_fits(digest_candidates(t, u), t.site_end > t.site_begin ? t.site_end - t.site_begin : 0, s.end - s.begin,
                            t.rare_end - t.rare_begin);
}

// Layout.  A tile's n representatives take digest_rows_padded(n) rows of the digest: granule g of its row i lies at dword
// (row_off wps) + (g P + i) 4, the last granule's r dwords at (row_off wps) + (G - 1) P 4 + i r, P the padded count — an SB64 block
// of P rows in place of 64, so the 64 rows a wave loads of one granule are contiguous, and every granule section starts on a
// 64-byte multiple of the tile's base.  Weights: uint16 per row at row_off + i.  Histogram: uint16[32 wps].
constexpr uint64_t DIGEST_ROW_GRAIN = 4;
IMPOP_TILE_HD inline uint64_t digest_rows_padded(uint64_t reps) { return (reps + DIGEST_ROW_GRAIN - 1) / DIGEST_ROW_GRAIN * DIGEST_ROW_GRAIN; }
inline uint64_t digest_hist_bytes(uint32_t wps) { return 64ull * wps; }
// a tile's singletons become a histogram unless its range of the stream reads fewer bytes
inline bool digest_takes_hist(const SingleRange &s, uint32_t wps) { return s.end > s.begin && single_bytes_streamed(s) >= digest_hist_bytes(wps); }

struct DigestLayout {
    std::vector<DigestDesc> descs;
    uint64_t n_rows = 0;        // representatives over all tiles
    uint64_t rows_padded = 0;   // rows of the digest
    uint64_t n_hist_tiles = 0;
    uint64_t row_bytes = 0, weight_bytes = 0, hist_bytes = 0;  // the three sections, in this order in one allocation
    uint64_t single_bytes = 0, entry_bytes = 0;                // kept ranges of the singleton stream; entries
    uint64_t digest_bytes() const { return row_bytes + weight_bytes + hist_bytes; }
    uint64_t weight_offset() const { return row_bytes; }  // a multiple of 16: rows_padded wps 4
    uint64_t hist_offset() const { return row_bytes + (weight_bytes + 15) / 16 * 16; }
    uint64_t alloc_bytes() const { return hist_offset() + hist_bytes; }
    // what a launch reads: rows (with their weights) and the rest (histograms, kept ranges, entries)
    uint64_t rows_streamed() const { return row_bytes + weight_bytes; }
    uint64_t rare_streamed() const { return hist_bytes + single_bytes + entry_bytes; }
    uint64_t bytes_streamed() const { return rows_streamed() + rare_streamed(); }
};
// reps[k]: tile k's representatives (the build's count pass); singles: empty on a route without the singleton stream
inline void digest_layout(const std::vector<ScanTile> &tiles, const std::vector<SingleRange> &singles, const uint32_t *reps, uint32_t wps,
                          DigestLayout &L) {
    L = DigestLayout();
    L.descs.resize(tiles.size());
    for (size_t k = 0; k < tiles.size(); ++k) {
        const SingleRange s = singles.empty() ? SingleRange{0, 0} : singles[k];
        DigestDesc &d = L.descs[k];
        d.row_off = L.rows_padded;
        d.n_rows = reps[k];
        d.rare_begin = tiles[k].rare_begin; d.rare_end = tiles[k].rare_end;
        if (digest_takes_hist(s, wps)) {
            d.hist = (uint32_t)++L.n_hist_tiles;
            d.single_begin = d.single_end = 0;
        } else {
            d.hist = 0;
            d.single_begin = s.begin; d.single_end = s.end > s.begin ? s.end : s.begin;
            L.single_bytes += single_bytes_streamed(s);
        }
        L.n_rows += reps[k];
        L.rows_padded += digest_rows_padded(reps[k]);
        L.entry_bytes += (tiles[k].rare_end - tiles[k].rare_begin) * 8ull;
    }
    L.row_bytes = L.rows_padded * 4ull * wps;
    L.weight_bytes = L.rows_padded * 2ull;
    L.hist_bytes = L.n_hist_tiles * digest_hist_bytes(wps);
}

// The default rule: a plan its maker will launch again (not the one-shot impop_scan: a plan launched once must not pay for the
// build), on the one-wave body, whose every tile fits, and whose launches read no more bytes with the digest than without — which
// also bounds the plan's memory by what the plan covers.  override: -1 none (the rule), 0 never, 1 whenever the body is the
// one-wave one and every tile fits (IMPOP_SCAN_DIGEST, read where a plan is made).
inline bool digest_wanted(int override_, bool reusable, bool wave_tiles, bool all_fit) {
    if (override_ == 0 || !wave_tiles || !all_fit) return false;
    return override_ == 1 || reusable;
}
inline bool digest_byte_rule(uint64_t digest_launch_bytes, uint64_t plain_launch_bytes) { return digest_launch_bytes <= plain_launch_bytes; }
inline bool digest_choice(int override_, bool reusable, bool wave_tiles, bool all_fit, uint64_t digest_launch_bytes, uint64_t plain_launch_bytes) {
    if (!digest_wanted(override_, reusable, wave_tiles, all_fit)) return false;
    return override_ == 1 || digest_byte_rule(digest_launch_bytes, plain_launch_bytes);
}

}  // namespace impop
