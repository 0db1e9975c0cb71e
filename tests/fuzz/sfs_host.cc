// sfs_host.cc — csrc/sfs_math.h on the host, under ASan + UBSan (tests/test_sfs_scan_host.py builds and runs it): the part cutter
// of impop_sfs_scan's table pass and its table-offset arithmetic, each against a brute-force model on random lists.
//   sfs_host parts <part_tiles> <t0> <t1> [<t0> <t1> ...]   prints the items of the windows: "items=N sizes=a,b,..."
//   sfs_host random <seed> <lists>                          random window lists and population panels; "random ok lists=N"
// The cutter's properties, checked on every list: every tile of every window lies in exactly one item of that window, the items
// of a window are in order and contiguous, no item is empty or longer than part_tiles, there are no more items than that bound needs and all
// but a window's last are ceil(tiles / items) long (equal shares), a window without tiles has no item, and sfs_part_count says how
// many there are.
// The offsets' properties: a table starts where the one before it ends, the row's length is the sum of the tables' bins, and
// every cell of every table has its own word of the row (a brute-force fill hits each word exactly once).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "sfs_math.h"

using namespace impop;

struct Win {
    uint64_t t0, t1;
};

static int fail(const char *what, size_t i) {
    fprintf(stderr, "ERROR: %s (at %zu)\n", what, i);
    return 1;
}

// 0 when the items are a correct cut of wins[w_begin, w_end)
static int check_parts(const std::vector<Win> &wins, uint64_t w_begin, uint64_t w_end, uint32_t part_tiles, const std::vector<SfsItem> &items) {
    const uint32_t cap = part_tiles < 1 ? 1 : part_tiles;
    size_t k = 0;
    uint64_t total = 0;
    for (uint64_t w = w_begin; w < w_end; ++w) {
        const uint64_t nt = wins[w].t1 > wins[w].t0 ? wins[w].t1 - wins[w].t0 : 0;
        std::vector<int> hits(nt, 0);  // the brute-force model: a counter per tile of the window
        uint64_t expect = wins[w].t0, n_items = 0;
        std::vector<uint64_t> lens;
        while (k < items.size() && items[k].win == w - w_begin) {
            const SfsItem &it = items[k];
            if (it.t1 <= it.t0) return fail("an empty item", k);
            if (it.t1 - it.t0 > cap) return fail("an item longer than part_tiles", k);
            if (it.t0 != expect) return fail("items of a window out of order or with a gap", k);
            if (it.t1 > wins[w].t1) return fail("an item past its window's tiles", k);
            for (uint32_t t = it.t0; t < it.t1; ++t) ++hits[t - wins[w].t0];
            lens.push_back(it.t1 - it.t0);
            expect = it.t1;
            ++n_items;
            ++k;
        }
        for (uint64_t t = 0; t < nt; ++t)
            if (hits[t] != 1) return fail("a tile that is not in exactly one item", (size_t)t);
        if (!nt && n_items) return fail("a window without tiles has an item", (size_t)w);
        if (n_items != sfs_part_count(nt, part_tiles)) return fail("sfs_part_count disagrees with the cut", (size_t)w);
        if (n_items != (nt + cap - 1) / cap) return fail("more items than the bound needs", (size_t)w);
        for (size_t j = 0; j + 1 < lens.size(); ++j)  // equal shares: all items but the last are ceil(nt / n_items) long
            if (lens[j] != (nt + n_items - 1) / n_items) return fail("items are not equal shares", (size_t)w);
        total += n_items;
    }
    if (k != items.size() || total != items.size()) return fail("items that belong to no window of the range", k);
    return 0;
}

static int check_offsets(const std::vector<uint32_t> &nk, const std::vector<uint32_t> &pairs) {
    const uint32_t K = (uint32_t)nk.size(), P = (uint32_t)(pairs.size() / 2);
    const SfsTableRows r = sfs_table_rows(nk.data(), K, pairs.data(), P);
    if (r.sfs_off.size() != K + 1 || r.jsfs_off.size() != P + 1) return fail("offset lists of the wrong length", 0);
    // brute force: write every cell of every table into a row, each word must be hit exactly once
    uint64_t len = 0;
    for (uint32_t k = 0; k < K; ++k) len += (uint64_t)nk[k] + 1;
    if (r.sfs_off[K] != len) return fail("the 1-D row's length", K);
    std::vector<uint8_t> row(len, 0);
    for (uint32_t k = 0; k < K; ++k)
        for (uint32_t c = 0; c <= nk[k]; ++c) {
            const uint64_t at = r.sfs_off[k] + c;
            if (at >= len || row[at]++) return fail("a 1-D bin outside the row or hit twice", k);
        }
    len = 0;
    for (uint32_t p = 0; p < P; ++p) len += ((uint64_t)nk[pairs[2 * p]] + 1) * ((uint64_t)nk[pairs[2 * p + 1]] + 1);
    if (r.jsfs_off[P] != len) return fail("the joint row's length", P);
    row.assign(len, 0);
    for (uint32_t p = 0; p < P; ++p) {
        const uint32_t na = nk[pairs[2 * p]], nb = nk[pairs[2 * p + 1]];
        uint64_t last = 0;
        for (uint32_t ca = 0; ca <= na; ++ca)
            for (uint32_t cb = 0; cb <= nb; ++cb) {
                const uint64_t bin = sfs_joint_bin(ca, cb, nb), at = r.jsfs_off[p] + bin;
                if ((ca || cb) && bin != last + 1) return fail("joint bins are not row-major in c_a", p);
                last = bin;
                if (at >= len || at >= r.jsfs_off[p + 1] || row[at]++) return fail("a joint cell outside its table or hit twice", p);
            }
    }
    return 0;
}

static uint64_t rnd(uint64_t &s) {
    s += 0x9E3779B97F4A7C15ull;
    uint64_t x = s;
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}

int main(int argc, char **argv) {
    if (argc < 2) return fail("usage: sfs_host parts|random ...", 0);
    const std::string mode = argv[1];
    if (mode == "parts") {
        if (argc < 3 || (argc - 3) % 2) return fail("parts <part_tiles> <t0> <t1> ...", 0);
        const uint32_t part_tiles = (uint32_t)strtoul(argv[2], nullptr, 10);
        std::vector<Win> wins;
        for (int i = 3; i + 1 < argc; i += 2) wins.push_back({strtoull(argv[i], nullptr, 10), strtoull(argv[i + 1], nullptr, 10)});
        std::vector<SfsItem> items;
        sfs_cut_parts(wins.data(), 0, wins.size(), part_tiles, items);
        if (check_parts(wins, 0, wins.size(), part_tiles, items)) return 1;
        printf("items=%zu sizes=", items.size());
        for (size_t k = 0; k < items.size(); ++k) printf("%s%u:%u", k ? "," : "", items[k].win, items[k].t1 - items[k].t0);
        printf("\n");
        return 0;
    }
    if (mode == "random") {
        if (argc != 4) return fail("random <seed> <lists>", 0);
        uint64_t s = strtoull(argv[2], nullptr, 10);
        const int lists = atoi(argv[3]);
        for (int l = 0; l < lists; ++l) {
            const uint64_t n_tiles = rnd(s) % 300;
            std::vector<Win> wins(rnd(s) % 40);
            for (Win &w : wins) {
                const uint64_t a = n_tiles ? rnd(s) % (n_tiles + 1) : 0, b = n_tiles ? rnd(s) % (n_tiles + 1) : 0;
                w = {a < b ? a : b, (rnd(s) & 7) ? (a < b ? b : a) : (a < b ? a : b)};  // one in eight without tiles
            }
            const uint32_t part_tiles = (uint32_t)(rnd(s) % 9);  // 0 counts as 1
            // a chunk of the list, as the call cuts it
            const uint64_t w0 = wins.empty() ? 0 : rnd(s) % (wins.size() + 1), w1 = w0 + (wins.empty() ? 0 : rnd(s) % (wins.size() + 1 - w0));
            std::vector<SfsItem> items;
            sfs_cut_parts(wins.data(), w0, w1, part_tiles, items);
            if (check_parts(wins, w0, w1, part_tiles, items)) return 1;
            std::vector<uint32_t> nk(1 + rnd(s) % 8), pairs;
            for (uint32_t &n : nk) n = 1 + (uint32_t)(rnd(s) % ((rnd(s) & 3) ? 12 : 70));
            const uint32_t P = nk.size() > 1 ? (uint32_t)(rnd(s) % 29) : 0;
            for (uint32_t p = 0; p < P; ++p) {
                const uint32_t a = (uint32_t)(rnd(s) % nk.size());
                uint32_t b = (uint32_t)(rnd(s) % nk.size());
                if (b == a) b = (a + 1) % (uint32_t)nk.size();
                pairs.push_back(a);
                pairs.push_back(b);
            }
            if (check_offsets(nk, pairs)) return 1;
        }
        printf("random ok lists=%d\n", lists);
        return 0;
    }
    return fail("unknown mode", 0);
}
