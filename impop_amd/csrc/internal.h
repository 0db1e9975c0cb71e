// internal.h — shared host-side structures of libimpop_hip.so (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>

#include "../../include/impop_hip.h"
#include "carve.h"
#include "tile_cut.h"

#define IMPOP_API extern "C" __attribute__((visibility("default")))

namespace impop {

void set_error(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
int hip_fail(hipError_t e, const char *what, const char *file, int line);

#define HIP_TRY(expr)                                                        \
    do {                                                                     \
        hipError_t _e = (expr);                                              \
        if (_e != hipSuccess) return impop::hip_fail(_e, #expr, __FILE__, __LINE__); \
    } while (0)

#define REQUIRE(cond, ...)                 \
    do {                                   \
        if (!(cond)) {                     \
            impop::set_error(__VA_ARGS__); \
            return IMPOP_E_INVALID;        \
        }                                  \
    } while (0)

// per-site outputs and the all-pairs path need every site: they refuse compacted matrices
#define NOT_COMPACT(m, fn)                                                                                     \
    do {                                                                                                       \
        if ((m)->compact) {                                                                                    \
            impop::set_error("%s: not available on a compacted matrix (impop_matrix_compact drops monomorphic sites)", fn); \
            return IMPOP_E_UNSUPPORTED;                                                                        \
        }                                                                                                      \
    } while (0)

void matrix_drop_derived(const impop_matrix *m);  // frees the lazily built weight planes / masked operand / site bitmap

#define NOT_WEIGHTED(m, fn)                                                                  \
    do {                                                                                     \
        if (!(m)->wt_prefix.empty()) {                                                                   \
            impop::set_error("%s: not available on a matrix with site weights", fn);         \
            return IMPOP_E_UNSUPPORTED;                                                      \
        }                                                                                    \
    } while (0)

// ---- SB64: site-blocked, wave-interleaved layout --------------------------------
// The site axis is cut into blocks of 64 sites (one wavefront).  A site holds
// wps = ceil(n_hap/32) dwords (dword k = haplotypes 32k..32k+31).  Inside a block the
// dwords are stored in 16-byte granules interleaved over the 64 sites, so that lane l
// of a wave (= site 64b+l) reads its granule g with ONE fully coalesced 1 KiB
// global_load_dwordx4:
//     dword(b, l, k) @ b*64*wps + (k/4)*256 + l*4 + (k%4)          for k/4 < G-1
//     dword(b, l, k) @ b*64*wps + (G-1)*256 + l*r + (k - 4(G-1))    last granule, r dwords
// with G = ceil(wps/4), r = wps - 4(G-1) in 1..4.  Bytes per site = 4*wps exactly
// (60 B for 465 haplotypes: 3.2 % above the algorithmic n/8).
struct SbGeom {
    uint32_t n_hap = 0;
    uint32_t wps = 0;    // dwords per site
    uint32_t G = 0;      // granules per site
    uint32_t r = 0;      // dwords in the last granule
    uint64_t n_site = 0;
    uint64_t n_block = 0;  // ceil(n_site/64)
};

// dword index of (block b, lane/site l, dword k) in the SB64 layout
__host__ __device__ inline uint64_t sb_index(uint32_t wps, uint32_t G, uint32_t r, uint64_t b, uint32_t l,
                                             uint32_t k) {
    const uint32_t g = k >> 2;
    const uint64_t base = b * 64ull * wps;
    return (g + 1 < G) ? base + (uint64_t)g * 256 + l * 4 + (k & 3)
                       : base + (uint64_t)(G - 1) * 256 + (uint64_t)l * r + (k - 4 * (G - 1));
}

// one-character environment switches (IMPOP_EPILOGUE_FAST=0, IMPOP_NO_POLARITY=1, ...): is the variable set and does it start with ch
inline bool env_is(const char *name, char ch) {
    const char *e = getenv(name);
    return e && e[0] == ch;
}
// IMPOP_TRACE=1: the calls' trace lines on stderr (read once per process)
inline bool trace_on() {
    static const bool on = env_is("IMPOP_TRACE", '1');
    return on;
}

// The timer of the batched calls: a pool of (start, stop) event pairs and the number of pairs COMPLETED since the last reset.
// A pair counts only once its stop event is recorded, so elapsed() never asks for an event that a failed launch left out.
// Bodies in context.hip.
struct EventPairs {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
    size_t done = 0;
    int begin(hipStream_t stream, size_t *slot);  // grows the pool if needed, records the start event of pair *slot
    int end(hipStream_t stream, size_t slot);     // records its stop event, then counts the pair
    void reset() { done = 0; }
    int elapsed(double *total_ms, uint64_t *launches) const;  // the stream must be synchronised; either pointer may be null
    void destroy();
};

// rare kept sites: min(c, n - c) <= IMPOP_RARE_MAX (one 8-byte entry lists their minor-allele carriers)
constexpr uint32_t IMPOP_RARE_MAX = 3;
// ---- the 8-byte rare entry of the split scan index (impop_matrix::d_vrare) ----
//     bits 0..1 = m (1..3 listed haplotypes), bit 15 = the listed haplotypes carry 0 (else 1), bits 16i+16..16i+31 = the index
//     of listed haplotype i (unused slots 0xFFFF); listed = carriers of the allele with count <= n/2, ties to the 1-allele.
constexpr uint64_t RARE_NO_SLOTS = 0xFFFFFFFFFFFF0000ull;  // every slot unused
__host__ __device__ inline uint32_t rare_count(uint64_t e) { return (uint32_t)e & 3u; }
__host__ __device__ inline bool rare_lists_zeros(uint64_t e) { return (e & 0x8000u) != 0; }
__host__ __device__ inline uint32_t rare_slot(uint64_t e, uint32_t i) { return (uint32_t)(e >> (16 * i + 16)) & 0xFFFFu; }
__host__ __device__ inline uint64_t rare_set_slot(uint64_t slots, uint32_t i, uint32_t h) {
    return (slots & ~(0xFFFFull << (16 * i + 16))) | ((uint64_t)h << (16 * i + 16));
}
__host__ __device__ inline uint64_t rare_pack(uint64_t slots, uint32_t m, bool zeros) { return slots | m | (zeros ? 0x8000u : 0u); }


// ---- the site classes of the scan index (impop_matrix::idx) ----
// KEPT: the variable sites, 0 < c < n.  COMMON: the kept sites with min(c, n - c) > IMPOP_RARE_MAX (split index).  SINGLE: the
// singleton sites, min(c, n - c) = 1 (singleton stream).  A class is built only on top of the one before it.
enum SiteClass { KEPT, COMMON, SINGLE, N_CLASS };
// Per 64-site block of the matrix, the mask of a class's sites and the number of them before the block: n_block + 1 entries
// each, one allocation, mask first; the last entry is {0, the total}.  mask null: the class was not built.
struct BlockRank {
    const uint64_t *mask = nullptr, *base = nullptr;
    // the sites of the class left of site s <= n_site, with no search
    __host__ __device__ uint64_t operator()(uint64_t s) const {
        return base[s >> 6] + (uint64_t)__builtin_popcountll(mask[s >> 6] & ((1ull << (s & 63)) - 1ull));
    }
};
struct ClassRanks {  // as a kernel argument
    BlockRank k[N_CLASS];
};
// what the kernels that write SB64 add for the index: per block, each wanted class's mask and its popcount (mask null: not wanted)
struct ClassOut {
    uint64_t *mask[N_CLASS] = {nullptr, nullptr, nullptr};
    uint32_t *cnt[N_CLASS] = {nullptr, nullptr, nullptr};
};

}  // namespace impop

struct impop_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    char arch[128] = {0};
    int n_cu = 0;
    // cached Tajima constants on the device, keyed by n (8 doubles: a1,a2,b1,b2,c1,c2,e1,e2): for the all-pairs calls, which
    // synchronise before they return.  Scan plans own their constants (impop_scan_plan::d_taj)
    double *d_taj = nullptr;
    int64_t taj_n = -1;
    uint32_t *d_queue = nullptr;  // 8 task-queue heads of the persistent Gram kernel
    // device error word (context.hip: ctx_err_word / ctx_err_fetch / ctx_err_result): kernels OR a bit in when an internal
    // invariant fails (stats.hip: the grouping's progress bound), the call that launched them returns IMPOP_E_INTERNAL
    uint32_t *d_err = nullptr;
    uint32_t h_err = 0;
    // impop_ctx_gram_timing: one switch, every timer (impop::EventPairs) in one array that reset and destroy walk
    bool gram_timing = false;
    enum Timer {
        T_GRAM,              // the Gram launch(es) of every chunk of impop_pairwise_scan / impop_cluster_scan (impop_ctx_gram_elapsed)
        T_CLUSTER,           // the clustering kernel(s) of impop_cluster_scan (impop_ctx_cluster_elapsed)
        T_EHH,               // the kernels of every chunk of impop_ehh_scan (impop_ctx_ehh_elapsed)
        T_HAP,               // impop_haplotype_scan: fingerprint / classify / verify + exact kernels (impop_ctx_haplotype_elapsed)
        T_LD = T_HAP + 3,    // impop_ld_scan: select / gather / pairs kernels (impop_ctx_ld_elapsed)
        T_DIP = T_LD + 3,    // impop_diploid_scan: tile / window kernels (impop_ctx_diploid_elapsed)
        T_DSTAT = T_DIP + 2, // impop_dstat_scan: the streaming launches (impop_ctx_dstat_elapsed)
        T_SFS,               // impop_sfs_scan: summary / table launches (impop_ctx_sfs_elapsed)
        T_IBS = T_SFS + 2,   // impop_ibs_scan: transpose / walk / combine + close kernels (impop_ctx_ibs_elapsed)
        T_PAIRDIST = T_IBS + 3,  // impop_pairdist_scan: the distribution kernel of every chunk (impop_ctx_pairdist_elapsed)
        T_IHS,               // impop_ihs_scan: classify + tables / walk kernels (impop_ctx_ihs_elapsed)
        T_KIN = T_IHS + 2,   // impop_genotypes_create's plane build / impop_kinship_scan's epilogue kernels (impop_ctx_kinship_elapsed)
        T_PCA = T_KIN + 2,   // impop_pca_scan: the eigen kernel of every chunk / the distance kernel (impop_ctx_pca_elapsed)
        T_PERM = T_PCA + 2,  // impop_permtest_scan: the preparation / labelling kernel of every chunk (impop_ctx_permtest_elapsed)
        T_IBD = T_PERM + 2,  // impop_ibd_scan: transpose / walk / combine + close / chain kernels (impop_ctx_ibd_elapsed)
        T_TREE = T_IBD + 4,  // impop_tree_scan: the tree kernel of every chunk (impop_ctx_tree_elapsed)
        T_RECOMB,            // impop_recomb_scan: select / gather / pairs / finish kernels (impop_ctx_recomb_elapsed)
        T_LDBAND = T_RECOMB + 4,  // impop_ldband_scan: select / rank + gather / pairs / prune / reduce kernels (impop_ctx_ldband_elapsed)
        T_PAINT = T_LDBAND + 5,   // impop_paint_scan: transpose / forward / backtrack + emit / window kernels (impop_ctx_paint_elapsed)
        T_COUNT = T_PAINT + 4
    };
    impop::EventPairs timers[T_COUNT];
    // side stream + fork/join events (created on first use): independent latency-bound epilogue kernels of the
    // all-pairs path run next to each other instead of one after the other
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // growable scratch
    void *scratch = nullptr;
    size_t scratch_bytes = 0;
    // growable PINNED host staging (context.hip ctx_pinned): per-chunk metadata up and records down of impop_pairwise_scan —
    // from pageable memory either copy is a host memcpy into the runtime's own staging buffer first (0.8 MB up before the Gram
    // kernel can start, 0.4 MB down after the last kernel, per 4096 windows)
    void *pinned = nullptr;
    size_t pinned_bytes = 0;
    // growable side buffers of the epilogue kernels that split large problems over several workgroups (stats.hip):
    // slot 0 h-fst partial sums, slot 1 pica2 group tables + row sums; separate because the two run side by side
    void *d_aux[2] = {nullptr, nullptr};
    size_t aux_bytes[2] = {0, 0};
};

struct impop_matrix {
    impop::SbGeom g;
    uint32_t *d_sb = nullptr;   // SB64 layout, n_block*64*wps dwords
    uint64_t sb_bytes = 0;
    // RB32 — row-group-blocked hap-major copy, operand layout of the Gram kernel (optional,
    // IMPOP_KEEP_HAP_MAJOR): rows are grouped by 32, sites by 64-site cells (2 dwords), and one
    // (group, cell) holds the 32 rows' dword pairs contiguously (256 B = one coalesced wave load):
    //     dword(row, d) @ (((row>>5) * rb_nb + (d>>1)) * 32 + (row&31)) * 2 + (d&1)
    uint32_t *d_rb = nullptr;
    uint64_t rb_nb = 0;         // cells per row group incl. 4 cells of slack (prefetch)
    uint32_t n_hap_pad = 0;     // rows padded to a multiple of 96 (zero rows; Gram tiles are 96 wide)
    // RB32 in minor-allele polarity (layout.hip sb_to_hm_kernel): row phi_row (= n_hap, inside the padding) holds the set of
    // complemented sites; 0xFFFFFFFF = stored as given (no padding row free: n_hap a multiple of 96; or IMPOP_NO_POLARITY=1)
    uint32_t phi_row = 0xFFFFFFFFu;
    uint64_t rb_bytes = 0;
    // compacted matrix (impop_matrix_compact): only the sites variable among all haplotypes were kept;
    // pos[k] = original index of kept site k (host copy for window mapping), n_site_orig = original length
    uint32_t *d_wt = nullptr;  // optional per-site weights (impop_matrix_set_site_weights), plain site order
    // weighted all-pairs path (pairwise.hip), built on first use: bit planes of the weights over 32-site dwords
    // (plane k, dword d: bit j = bit k of weight[32 d + j]) and one masked copy of the RB32 operand
    mutable uint32_t *d_wplanes = nullptr;
    mutable uint32_t wplane_bits = 0;     // planes that have any bit set
    mutable uint64_t wplane_stride = 0;   // dwords per plane
    mutable uint32_t *d_rb_masked = nullptr;
    // lazily built bitmap of the sites that segregate among ALL haplotypes (bit s of dword s>>5), cached for the
    // all-pairs path's S (pairwise.hip); dropped with the matrix
    mutable uint32_t *d_segmap = nullptr;
    // compacted matrix: bitmap, in ORIGINAL site coordinates, of the dropped sites that EVERY haplotype carries (c_s = n):
    // each adds 1 to every I_ij, so the all-pairs path on the variable sites alone plus this per-window count is exact
    // (pairwise.hip, which also needs d_rb: a source that kept its hap-major copy); likewise every individual's hom_alt (diploid.hip)
    uint32_t *d_onesmap = nullptr;
    uint64_t *d_pos = nullptr;  // compacted: device copy of `pos` (map_windows_device: window edges -> kept-site indices on the GPU)
    bool compact = false;
    uint64_t n_site_orig = 0;
    std::vector<uint64_t> pos;
    std::vector<uint64_t> pos_coarse;  // pos[k << POS_COARSE_SHIFT]: a cache-resident first level for pos_lower_bound
    // compacted from a WEIGHTED matrix that kept its hap-major copy (all-pairs path): prefix sums, in ORIGINAL coordinates, of
    // the weights of the dropped sites every haplotype carries (a window's constant `add`), and of the kept columns' weights
    std::vector<uint64_t> ones_wt_prefix, kept_wt_prefix;
    std::vector<uint64_t> wt_prefix;  // weighted: prefix sums of the (ORIGINAL, if compacted) site weights, n + 1 entries
    // variable-site scan index (layout.hip index_begin / index_finish), built with every full matrix unless the caller opts out
    // (IMPOP_KEEP_DENSE_SCAN): the sites that vary among ALL haplotypes (0 < c < n) as an SB64 copy of their own (geometry vg:
    // the matrix's wps / G / r, n_site = the number kept, the same slack block), plus the per-block rank table of the kept sites,
    // idx[KEPT], so a window edge s maps in O(1) to kept(s) = idx[KEPT](s).  Scan plans of an unweighted matrix stream d_vsb
    // instead of d_sb (scan.hip); what the index holds depends on the matrix alone.
    uint32_t *d_vsb = nullptr;                         // null: no index (vskip says why)
    impop::BlockRank idx[impop::N_CLASS];              // one allocation per class
    impop::SbGeom vg;
    uint64_t vsb_bytes = 0, vidx_bytes = 0;            // kept-site SB64 without slack; everything the index allocated
    uint64_t n_vkept = 0;                              // variable sites (rare + common when split)
    std::string vskip = "not built";
    // rare/common split of the index (layout.hip rare_entries_kernel): a kept site is RARE when min(c, n - c) <= IMPOP_RARE_MAX.
    // Then d_vsb (geometry vg) holds the COMMON kept sites only, and d_vrare one 8-byte entry per rare site in site order
    // (format: rare_pack and its readers above).  idx[COMMON] ranks the common sites; rare(s) = kept(s) - common(s).
    // d_vrare null: no split (rskip says why), d_vsb holds every kept site as before.
    uint64_t *d_vrare = nullptr;
    uint64_t n_vrare = 0;
    std::string rskip = "not built";
    // singleton stream of the split index (layout.hip rare_entries_kernel; built for wps <= 16, the range of its one consumer,
    // the fixed-WPS scan kernel): the rare sites once more, as two packed streams in site order.  d_vsingle holds one uint16 per
    // SINGLETON site, min(c, n - c) = 1: bits 0..14 = the one carrier of the minor allele, bit 15 = that haplotype carries 0 (the
    // meaning of bit 15 of an 8-byte entry); padded with 0xFFFF to a multiple of 8 bytes plus 8 bytes of slack, so aligned 8-byte
    // loads of any range stay inside the allocation.  d_vmulti holds the other rare sites (min(c, n - c) = 2 or 3) as 8-byte
    // entries (rare_pack).  idx[SINGLE] ranks the singleton sites; multi(s) = rare(s) - single(s).  d_vrare stays complete.
    // d_vsingle null: no stream (sskip says why).
    uint16_t *d_vsingle = nullptr;
    uint64_t *d_vmulti = nullptr;
    uint64_t n_vsingle = 0, vsingle_bytes = 0;  // singleton sites; everything the stream allocated
    std::string sskip = "not built";
    // distinct-row stream of the split index (layout.hip unique_rows_build; wps <= 16, the range of its one reader, the fixed-WPS
    // scan kernel; independent of the singleton stream).  Per 64-row block of d_vsb, rows that are equal or each other's
    // complement within the n_hap real haplotypes form a class (every scan sum and segregating test is the same for a row and its
    // complement); the class's first row is its REPRESENTATIVE and its weight the number of rows of the class, 1..64.  d_vuniq is
    // an SB64 layout (the matrix's wps / G / r, zero rows to the end of the last block, one block of slack) of the representatives'
    // rows as d_vsb stores them, in order, so a block's representatives are contiguous; d_vuniq_wt holds one weight byte per
    // representative (zeros to the end of the last block plus 64 bytes of slack: a wave's 64-byte load of any block stays inside).
    // uidx ranks the representatives in COMMON-ROW coordinates: per block of d_vsb the mask of its representatives and the number
    // of them before the block, vg.n_block + 1 entries each.  Kept only when it pays: representatives <= 3/4 of the common rows.
    // d_vuniq null: no stream (uskip says why).  d_vsb stays complete.
    uint32_t *d_vuniq = nullptr;
    uint8_t *d_vuniq_wt = nullptr;
    impop::BlockRank uidx;
    uint64_t n_vuniq = 0, vuniq_bytes = 0;  // representatives; everything the stream allocated
    std::string uskip = "not built";
    int device = 0;
    mutable int users = 0;      // live scan plans referencing this matrix (impop_matrix_free refuses while > 0)
};

namespace impop {
int ctx_scratch(impop_ctx *ctx, size_t bytes, void **out);
int ctx_pinned(impop_ctx *ctx, size_t bytes, void **out);  // host, page-locked, grow-only; valid until the next larger request
int ctx_err_fetch(impop_ctx *ctx);                 // enqueue its copy to the host (before the call's own stream sync)
int ctx_err_result(impop_ctx *ctx, const char *fn);  // after that sync: IMPOP_OK, or IMPOP_E_INTERNAL (word cleared, message set)
// the impop_ctx_*_elapsed readers: syncs the stream, then timers[first + k] -> kernel_ms[k] for k < n (kernel_ms nullable);
// *count (nullable) = the completed pairs of timers[first + which]
int ctx_timers_elapsed(impop_ctx *ctx, int first, int n, int which, double *kernel_ms, uint64_t *count);
constexpr uint32_t DEV_ERR_GROUPING = 1u;            // greedy_groups_bits ran out of its progress bound
constexpr uint32_t DEV_ERR_CLUSTER = 2u;             // af label propagation ran out of its rounds
constexpr uint32_t DEV_ERR_HAPSCAN = 8u;             // haplotype scan: the classes of a window do not partition its members
constexpr uint32_t DEV_ERR_LDSCAN = 16u;             // LD scan: the rows gathered for a window are not its n_used
constexpr uint32_t DEV_ERR_DIPLOID = 32u;           // diploid scan: a window's rows do not add up to its het_total or its length
constexpr uint32_t DEV_ERR_IBS = 64u;               // IBS scan: a pair's runs do not add up to the range, or the fill met a tract the count did not announce
constexpr uint32_t DEV_ERR_IHS = 128u;              // iHS scan: a class's break weights do not add up to its pairs, or a reach lies in front of the warm-up start
constexpr uint32_t DEV_ERR_KINSHIP = 256u;          // kinship scan: a cell of a pair's joint genotype table came out negative
constexpr uint32_t DEV_ERR_PERMTEST = 512u;         // permutation test: the matrix-core path's values of the observed labelling are not the direct ones
constexpr uint32_t DEV_ERR_IBD = 1024u;             // IBD scan: the fill met a segment the count did not announce, or fewer than it announced
constexpr uint32_t DEV_ERR_RECOMB = 2048u;         // recombination scan: a window's gathered rows are not its n_used, or rmin exceeds the sites that have an incompatible left neighbour
constexpr uint32_t DEV_ERR_LDBAND = 4096u;         // banded LD scan: a window's gathered rows are not its q, it keeps more sites than it has, or its site rows do not add up to twice its record
constexpr uint32_t DEV_ERR_PAINT = 8192u;          // painting: a path's recomputed cost is not the forward pass's, its segments do not tile the range, or the emit met a segment the count did not announce
constexpr uint32_t DEV_ERR_EHH = 4u;                // ehh partition refinement ended with classes that do not account for the unbroken pairs
int ctx_aux(impop_ctx *ctx, int slot, size_t bytes, void **out);
// stats.hip: seed_rank -> order (inverse permutation) restricted to `members` (positions 0..m of the member list); ranks only need
// to be distinct among the members, else IMPOP_E_INVALID with *dup = a rank that occurs twice (the caller words the message)
int seed_order_of(const uint32_t *seed_rank, const uint32_t *members, uint32_t m, std::vector<uint32_t> &order, uint32_t *dup);
// context.hip: fork the side stream (created with its two events on first use) off ctx->stream, run `body` with ctx->stream
// pointing at it, record ev_join behind what it enqueued.  ctx->stream is the caller's again on every path, errors included;
// the caller joins where it needs the results: hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0)
int on_side_stream(impop_ctx *ctx, const std::function<int()> &body);
// pairwise.hip: build (once) the bitmap of the sites that segregate among all haplotypes, m->d_segmap
int ensure_segmap(impop_ctx *ctx, const impop_matrix *m);
// pairwise.hip, for the windowed calls of pairwise_scan.hip
struct GramWindow {
    uint64_t site_begin, site_end;
};
// Gram matrices of `n_win` cells (host copy h_wins of d_wins for the cell range) into d_out.  out16 (in / out, nullable): the
// caller would take uint16 counts (every window's W < 65536); set to whether the launch wrote them
int launch_gram_any(impop_ctx *ctx, const impop_matrix *m, const GramWindow *d_wins, const GramWindow *h_wins, uint32_t n_win,
                    int32_t *d_out, uint64_t max_window_sites, bool *out16 = nullptr);
int launch_gram_unflip(impop_ctx *ctx, const impop_matrix *m, int32_t *d_g, uint64_t n_mats, bool g16 = false);
// popcount of a site bitmap over each window -> s_all and s_p of d_stats[w] and / or d_plain[w] (either nullable)
int launch_seg_count(impop_ctx *ctx, const uint32_t *d_map, const GramWindow *d_wins, uint64_t n_win, impop_window_stats *d_stats,
                     uint32_t *d_plain);
int check_pairwise_args(impop_ctx *ctx, const impop_matrix *m, uint64_t s0, uint64_t s1, const char *fn);
// W of a window: its length, or the sum of its columns' weights
inline uint64_t window_W(const impop_matrix *m, uint64_t s0, uint64_t s1) {
    return m->wt_prefix.empty() ? s1 - s0 : m->wt_prefix[s1] - m->wt_prefix[s0];
}
// compacted from a weighted matrix: the summed weights of the dropped all-ones sites of [s0, s1) (original coordinates)
inline uint32_t ones_weight(const impop_matrix *m, uint64_t s0, uint64_t s1) {
    return (uint32_t)(m->ones_wt_prefix[s1] - m->ones_wt_prefix[s0]);  // < 2^31: part of the window's W
}
inline bool compact_weighted(const impop_matrix *m) { return m->compact && !m->ones_wt_prefix.empty(); }
int ensure_tajima_consts(impop_ctx *ctx, int64_t n);  // fills ctx->d_taj for n (device kernel)
// the same kernel into a slot of the caller's (8 doubles), on the context's stream: a scan plan's own constants, which no other
// plan or call on the context retargets (a captured launch reads its slot at replay time)
int fill_tajima_consts(impop_ctx *ctx, int64_t n, double *d_out);
// scan.hip: impop_scan_plan_create for the library's own calls.  reusable = false: the plan is launched once, and the default
// rule leaves it without a tile digest (tile_digest.h: a plan launched once must not pay for the build)
int scan_plan_create(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows, const uint64_t *mask_p,
                     const uint64_t *mask_a, const uint64_t *mask_b, const impop_scan_params *params, bool reusable, impop_scan_plan **out);

// windows are given in ORIGINAL site coordinates; for a compacted matrix map them to kept-site index
// ranges (`mapped`), else `mapped` is a plain copy.  span() = the coordinate range windows must lie in.
inline uint64_t matrix_span(const impop_matrix *m) { return m->compact ? m->n_site_orig : m->g.n_site; }
void map_windows(const impop_matrix *m, const impop_window *windows, uint64_t n, std::vector<impop_window> &mapped);
// the same on the device (one thread per window edge, binary search in the device copy of the positions): 8192 searches over
// 87 MB of positions cost the host 0.55 ms per call — as long as the Gram launch they precede — and the GPU some 50 us
int map_windows_device(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n, std::vector<impop_window> &mapped);
// compacted matrices: index of the first kept site at or right of original coordinate s (= number of kept sites left of s)
uint64_t pos_lower_bound(const impop_matrix *m, uint64_t s);
constexpr unsigned POS_COARSE_SHIFT = 12;

// variable-site scan index: window edges in matrix coordinates -> kept-site index ranges of d_vsb (one thread per edge, no search)
// the index a kept fraction above 1/IMPOP_INDEX_MAX_KEPT_INV of the sites is not built for (the dense stream is then nearly as short)
constexpr uint64_t IMPOP_INDEX_MAX_KEPT_INV = 4;
// top = the last class wanted: KEPT gives kept-site ranges (r = g = 0), COMMON common-site ranges and the rare entries
// between them (r = kept(s) - common(s)), SINGLE also the singletons (g = single(s)) and r = multi(s) = rare(s) - single(s)
int map_windows_index(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n, SiteClass top,
                      std::vector<LayoutWindow> &out);

// layout.hip
// idx: also write the masks and counts of the classes it names (scan index)
int launch_hm_to_sb(impop_ctx *ctx, const uint32_t *d_hm, uint64_t hm_stride, const SbGeom &g, uint32_t *d_sb, const ClassOut &idx = ClassOut());
// rb_nb == 0: plain hap-major rows of hm_stride dwords; else RB32 addressing with rb_nb cells per row group
int launch_sb_to_hm(impop_ctx *ctx, const uint32_t *d_sb, const SbGeom &g, uint64_t blk_begin, uint64_t blk_end,
                    uint32_t *d_hm, uint64_t hm_stride, uint32_t n_rows, uint64_t rb_nb = 0, uint32_t phi_row = 0xFFFFFFFFu);

}  // namespace impop
