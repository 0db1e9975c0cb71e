// win_chunks.h — the host arithmetic the chunked window calls share (impop_haplotype_scan, impop_ld_scan, impop_diploid_scan,
// impop_ehh_scan): who is a member, and which windows go into which chunk.  Plain C++, no HIP: tests/fuzz/win_chunks.cc compiles
// it on the host under the sanitizers and checks every plan against a brute-force model.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace impop {

// The haplotypes a mask selects (bitset of ceil(n_hap / 64) words; null: everyone; bits at or above n_hap are ignored).
// (K disjoint masks as panels — classes, positions, merged pairs — are panel_set.h, built on this.)
struct MemberSet {
    std::vector<uint32_t> idx;   // the members, ascending
    std::vector<int32_t> ppos;   // wps * 32 entries: a member's position in idx, -1 for everyone else (padding rows included)
    std::vector<uint32_t> bits;  // wps dwords: bit i & 31 of dword i >> 5 = i is a member
    uint32_t size() const { return (uint32_t)idx.size(); }
};
inline MemberSet member_set(const uint64_t *mask, uint32_t n_hap, uint32_t wps) {
    MemberSet s;
    s.ppos.assign((size_t)wps * 32, -1);
    s.bits.assign(wps, 0u);
    for (uint32_t i = 0; i < n_hap; ++i)
        if (!mask || ((mask[i >> 6] >> (i & 63)) & 1ull)) {
            s.ppos[i] = (int32_t)s.idx.size();
            s.bits[i >> 5] |= 1u << (i & 31);
            s.idx.push_back(i);
        }
    return s;
}

// max_chunk_bytes of a call's params: 0 = the default of 1 GiB
inline uint64_t chunk_budget(uint64_t max_chunk_bytes) { return max_chunk_bytes ? max_chunk_bytes : (1ull << 30); }

// the largest f(chunk), at least `floor` (what a launch or a sub-buffer must hold)
template <typename Chunks, typename F>
size_t max_over(const Chunks &chunks, F f, size_t floor = 1) {
    size_t mx = floor;
    for (const auto &c : chunks) mx = std::max<size_t>(mx, (size_t)f(c));
    return mx;
}

struct WinChunk {
    uint64_t w_begin = 0, w_end = 0;  // windows [w_begin, w_end) of the call's list
};

// The greedy cut: windows in order, a chunk taking the next one while its bytes stay within the budget and its windows within
// win_cap (0: no cap).  A chunk always takes one window: a window alone may exceed the budget.  add(c, i) = the bytes window i
// would add to chunk c as it stands; take(c, i), if given, tells the caller that it went in.  add must not change the caller's
// state: the window it is asked about may open the next chunk instead.  take(c, .) is called at least once for every chunk c.
template <typename Add, typename Take = void (*)(size_t, uint64_t)>
std::vector<WinChunk> cut_windows(uint64_t n_windows, uint64_t budget, uint64_t win_cap, Add add, Take take = [](size_t, uint64_t) {}) {
    std::vector<WinChunk> out;
    for (uint64_t i = 0; i < n_windows;) {
        WinChunk c;
        c.w_begin = i;
        uint64_t bytes = 0;
        for (; i < n_windows; ++i) {
            const uint64_t a = add(out.size(), i);
            if (i > c.w_begin && (bytes + a > budget || (win_cap && i - c.w_begin == win_cap))) break;
            take(out.size(), i);
            bytes += a;
        }
        c.w_end = i;
        out.push_back(c);
    }
    return out;
}

// ---- chunks of windows over shared tiles: a tile is paid for once per chunk, by the first window of the chunk that holds it
struct TileCosts {
    uint64_t per_tile, per_win, per_item;  // device bytes per fresh tile, per window, per (window, tile) item
};
struct TiledChunk : WinChunk {
    std::vector<uint64_t> tiles;  // the tiles of its windows, each once, ascending: every window's range stays contiguous
    std::vector<uint32_t> l0;     // per window: its first tile's place in `tiles` (0 for a window without tiles)
    uint64_t items = 0;           // (window, tile) pairs
};
// wins: anything with a tile range [t0, t1) inside [0, n_tiles)
template <typename Win>
std::vector<TiledChunk> plan_tiled_chunks(const Win *wins, uint64_t n_windows, uint64_t n_tiles, uint64_t budget, uint64_t win_cap,
                                          const TileCosts &k) {
    std::vector<uint64_t> seen(n_tiles, 0);  // the last chunk (+ 1) that took the tile
    std::vector<uint32_t> local(n_tiles, 0u);
    std::vector<std::vector<uint64_t>> used;
    const std::vector<WinChunk> cuts = cut_windows(
        n_windows, budget, win_cap,
        [&](size_t c, uint64_t i) {
            uint64_t fresh = 0;
            for (uint64_t t = wins[i].t0; t < wins[i].t1; ++t) fresh += seen[t] != c + 1;
            return fresh * k.per_tile + k.per_win + (wins[i].t1 - wins[i].t0) * k.per_item;
        },
        [&](size_t c, uint64_t i) {
            if (used.size() <= c) used.emplace_back();
            for (uint64_t t = wins[i].t0; t < wins[i].t1; ++t)
                if (seen[t] != c + 1) {
                    seen[t] = c + 1;
                    used[c].push_back(t);
                }
        });
    std::vector<TiledChunk> out(cuts.size());
    for (size_t c = 0; c < cuts.size(); ++c) {
        TiledChunk &o = out[c];
        o.w_begin = cuts[c].w_begin;
        o.w_end = cuts[c].w_end;
        o.tiles.swap(used[c]);
        std::sort(o.tiles.begin(), o.tiles.end());
        for (size_t j = 0; j < o.tiles.size(); ++j) local[o.tiles[j]] = (uint32_t)j;
        o.l0.reserve(o.w_end - o.w_begin);
        for (uint64_t i = o.w_begin; i < o.w_end; ++i) {
            o.l0.push_back(wins[i].t1 > wins[i].t0 ? local[wins[i].t0] : 0u);
            o.items += wins[i].t1 - wins[i].t0;
        }
    }
    return out;
}

}  // namespace impop
