/*
 * impop_hip.h — C ABI of libimpop_hip.so: the MI355X (gfx950) windowed
 * population-statistics engine for impop's pairwise-diversity hot path.
 *
 * The reference (pangenome/impop) has no FFI: the path sits behind Python
 * functions and CLIs.  Each entry point below names the
 * reference interface it replaces (file:line relative to the reference root).
 * The reference-side binding a maintainer would add is the ctypes stub shown in
 * INTEGRATION.md; impop_amd/_lib.py is exactly that stub.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes only; no exceptions, no Python or
 *    torch types cross the boundary.
 *  - every function returns 0 on success or a negative impop_status; the
 *    message is retrievable with impop_last_error() (thread-local).
 *  - a context (impop_ctx) owns one HIP stream on one device; it is not
 *    thread-safe, the library is re-entrant across contexts.
 *  - host pointers are caller-owned; device memory lives behind opaque handles.
 *  - haplotypes are indexed 0..n-1 in the caller's order; for the name-ordered
 *    semantics of pica2.py/af.py the caller passes them in lexicographic name
 *    order (the Python layer does).
 *  - dense identity matrices are row-major double[n*n]; NaN marks a pair that
 *    is absent from the .sim table (pica2.py:131-134, h-fst.py:152-153).
 *  - all compute runs on the GPU; there is no CPU fallback.  Without a usable
 *    gfx950 device impop_ctx_create fails with IMPOP_E_NODEVICE.
 */
#ifndef IMPOP_HIP_H
#define IMPOP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IMPOP_ABI_VERSION 4

typedef enum impop_status {
    IMPOP_OK = 0,
    IMPOP_E_INVALID = -1,   /* bad argument (also the reference's ValueError cases, tj_d.py:48-51) */
    IMPOP_E_NODEVICE = -2,  /* no HIP device / wrong architecture */
    IMPOP_E_HIP = -3,       /* a HIP runtime call failed */
    IMPOP_E_NOMEM = -4,
    IMPOP_E_UNSUPPORTED = -5,
    IMPOP_E_INTERNAL = -6   /* a device-side consistency check tripped (results of the call are not to be used) */
} impop_status;

typedef struct impop_ctx impop_ctx;
typedef struct impop_matrix impop_matrix;
typedef struct impop_scan_plan impop_scan_plan;

/* ---- library / context -------------------------------------------------- */
int impop_version(void);                 /* IMPOP_ABI_VERSION */
const char *impop_last_error(void);      /* thread-local, never NULL */
int impop_device_count(int *count);
/* stream: an existing hipStream_t created by the caller (its ordering is then the caller's: collectives
 * and copies issued on it see the scans), or NULL to create a private non-blocking stream.  NULL is also
 * HIP's legacy null stream — it cannot be adopted; a caller that works on the null stream (torch's default
 * stream reports handle 0) must create an explicit stream and pass that. */
int impop_ctx_create(int device, void *stream, impop_ctx **out);
int impop_ctx_destroy(impop_ctx *ctx);
int impop_ctx_synchronize(impop_ctx *ctx);
/* device name/arch string of the context's device, e.g. "gfx950:sramecc+:xnack-" */
int impop_ctx_device_name(impop_ctx *ctx, char *buf, size_t buflen);

/* ---- presence matrix ------------------------------------------------------
 * Replaces the per-window `impg similarity` -> .sim TSV -> read_similarity_file
 * round trip (run_pica2_impg.sh:162-175, pica2.py:6-58, h-fst.py:84-119): the
 * haplotype x site presence matrix stays resident in HBM.
 *
 * Interchange layout ("hap-major"): bits[i*row_stride_words + (s>>6)] bit (s&63)
 * is 1 iff haplotype i carries the allele at site s.
 * keep flags: which device layouts to materialise. */
#define IMPOP_KEEP_SITE_BLOCKED 1u /* SB64 layout used by impop_scan (always kept) */
#define IMPOP_KEEP_HAP_MAJOR 2u    /* haplotype-major (row-group-blocked) copy needed by impop_pairwise_* */
/* Opt out of the variable-site scan index.  Without this flag every matrix made by impop_matrix_upload /
 * impop_matrix_synthetic[_slab] also gets, built on the device when it is made, a second SB64 layout of the sites
 * that vary among ALL haplotypes (0 < c_s < n) plus, per 64-site block, the mask of those sites and the number
 * kept before it.  A monomorphic site adds 0 to every sum_s c(n-c) of every subset and segregates in none, so
 * impop_scan / impop_scan_plan_* / impop_scan_multi / impop_scan_sharded on an unweighted matrix stream the kept
 * sites only and return the records of the dense stream, byte for byte (window edges map in O(1); n_sites stays the
 * window's length).  The index depends on the matrix alone, not on windows or masks.  It is not built when more
 * than 1/4 of the sites vary (the dense stream is then barely longer) or when its device memory cannot be had (the
 * matrix is made all the same); impop_matrix_scan_index_info says which.  Weighted matrices (site weights are
 * indexed by matrix site) always stream the dense layout; impop_afs, impop_site_counts, impop_ehh, download and the
 * all-pairs path never use the index.  impop_matrix_info's device_bytes does not count it. */
#define IMPOP_KEEP_DENSE_SCAN 4u
/* The index is also split, when it is built and n_hap is 65..65535: a kept site with min(c, n - c) <= 3 (a RARE site) is
 * stored as one 8-byte entry listing its minor-allele carriers, and only the other (COMMON) kept sites as SB64 rows.  Scans
 * read both streams and return the same records.  IMPOP_KEEP_NO_RARE_SPLIT keeps every kept site as a row (the unsplit
 * index); impop_matrix_scan_split_info reports the split, or why there is none. */
#define IMPOP_KEEP_NO_RARE_SPLIT 8u
/* A split index of a matrix of 65..512 haplotypes also keeps its rare sites as two packed streams, which the plans of
 * impop_scan_plan_create read instead of the 8-byte entries: one uint16 per SINGLETON site (min(c, n - c) = 1: the index of
 * its one minor-allele carrier) and the 8-byte entries of the other rare sites alone.  Records do not change; a launch
 * reads 2 bytes per singleton instead of 8.  Every other call keeps reading the 8-byte entries, which stay complete.
 * IMPOP_KEEP_NO_SINGLE_STREAM leaves the two streams out; impop_matrix_scan_single_info reports them, or why there are none. */
#define IMPOP_KEEP_NO_SINGLE_STREAM 16u
/* A split index of 65..512 haplotypes also keeps, per 64-row block of its common rows, the DISTINCT rows once with a one-byte
 * multiplicity: rows that are equal, or each other's complement within the n_hap haplotypes (every sum and segregating test of
 * a scan is the same for a row and its complement), are one representative of weight 1..64.  Plans of impop_scan_plan_create
 * read the whole blocks of a tile from this stream and only the partial blocks at window edges as rows; records do not change.
 * The stream is kept only where it pays (representatives at most 3/4 of the common rows) and costs nothing elsewhere; every
 * other call keeps reading the rows, which stay complete.  IMPOP_KEEP_NO_UNIQUE_ROWS leaves it out (as does IMPOP_NO_UNIQUE_ROWS=1
 * in the environment, for every matrix of the process); impop_matrix_scan_unique_info reports it, or why there is none. */
#define IMPOP_KEEP_NO_UNIQUE_ROWS 32u

int impop_matrix_upload(impop_ctx *ctx, const uint64_t *bits_hap_major, uint32_t n_hap, uint64_t n_site,
                        uint64_t row_stride_words, uint32_t keep_flags, impop_matrix **out);

/* Synthetic matrix generated on the device (bench / tests; SURVEY.md §8d
 * generator re-expressed as a counter-based hash so any window can be
 * regenerated independently on the CPU): ancestral allele per site, n_founder
 * lineages each differing at p_founder of sites, per-32-haplotype-word private
 * flips with probability p_private_word. */
typedef struct impop_synth_params {
    uint64_t seed;
    uint32_t n_founder;       /* 1..32 */
    double p_founder;         /* per founder per site */
    double p_private_word;    /* per (site, 32-haplotype word): one random bit flips */
} impop_synth_params;
int impop_matrix_synthetic(impop_ctx *ctx, uint32_t n_hap, uint64_t n_site, const impop_synth_params *p,
                           uint32_t keep_flags, impop_matrix **out);
/* Sites [site_begin, site_begin + n_site) of the same synthetic chromosome (the generator is counter-based on the global
 * site index): what a rank of a sharded scan holds — its window range's slab plus halo — without anybody
 * ever materialising the whole matrix.  Site 0 of the returned matrix is global site `site_begin`. */
int impop_matrix_synthetic_slab(impop_ctx *ctx, uint32_t n_hap, uint64_t site_begin, uint64_t n_site,
                                const impop_synth_params *p, uint32_t keep_flags, impop_matrix **out);

/* Copy sites [site_begin, site_end) back to the host in hap-major layout
 * (bit 0 of word 0 of each row = site_begin). */
int impop_matrix_download(impop_ctx *ctx, const impop_matrix *m, uint64_t site_begin, uint64_t site_end,
                          uint64_t *bits_hap_major_out, uint64_t row_stride_words);
/* Optional per-site weights (NULL removes them): column s stands for weights[s] base pairs, e.g. one
 * column per graph node with the node's length, instead of repeating the column per bp.  impop_scan /
 * impop_scan_plan_* then return sum_s w_s c(n-c) sums and n_sites = sum_s w_s over the window — the
 * records of the bp-expanded matrix — while s_all / s_p / s_a / s_b keep counting COLUMNS (variable nodes,
 * what a VCF of the window lists, run_tajd.sh:148).  impop_matrix_compact keeps the weights (a window's W stays
 * the sum over all its original columns); impop_scan_multi honours them too.  Set them before building plans
 * (refused while plans of this matrix are alive).  The all-pairs path (impop_pairwise_*) honours them as well:
 * I_ij = sum_s w_s b_is b_js — the bp-weighted node-sharing counts behind `impg similarity`'s identity
 * (run_pica2_impg.sh:162-175) — W = sum_s w_s, computed exactly through the weights' bit planes
 * (I = sum_k 2^k Gram(M & W_k)); a window's summed weights must stay below 2^31. */
int impop_matrix_set_site_weights(impop_ctx *ctx, impop_matrix *m, const uint32_t *weights_host);

/* Keep only the sites that are variable among ALL haplotypes (0 < c_s < n), with their original
 * positions.  Monomorphic sites add 0 to every sum_s c(n-c) of every subset and are never segregating
 * (what `povu gfa2vcf | wc -l` counts, run_tajd.sh:148), so impop_scan / impop_scan_plan_* /
 * impop_scan_multi on the compacted matrix, given windows in the ORIGINAL site coordinates, return
 * records identical to those of the full matrix (n_sites = the window's original length) while
 * streaming only the variable sites.  When `m` kept its hap-major copy (IMPOP_KEEP_HAP_MAJOR), the compacted matrix
 * serves the all-pairs path too: a dropped site that NO haplotype carries adds nothing to any I_ij, one that EVERY
 * haplotype carries adds exactly 1 — its weight w_s on a weighted matrix — to every I_ij (diagonal included), so
 * impop_pairwise_* contract the kept sites of a window only and add the window's count of dropped all-ones sites (a
 * bitmap in original coordinates; for a weighted source, host prefix sums of their weights) — identical counts,
 * identities and records from W/S times fewer multiply-adds, and on node-level matrices without the long shared
 * anchors' weight planes.
 * Per-site outputs (impop_afs, impop_site_counts, impop_ehh) return IMPOP_E_UNSUPPORTED on a compacted matrix. */
int impop_matrix_compact(impop_ctx *ctx, const impop_matrix *m, impop_matrix **out);
/* original site index of kept sites [first, first+count) of a compacted matrix; n_site_orig (nullable)
 * receives the original number of sites */
int impop_matrix_positions(const impop_matrix *m, uint64_t first, uint64_t count, uint64_t *positions_out,
                           uint64_t *n_site_orig);
int impop_matrix_info(const impop_matrix *m, uint32_t *n_hap, uint64_t *n_site, uint64_t *device_bytes,
                      uint32_t *bytes_per_site);
/* The variable-site scan index (see IMPOP_KEEP_DENSE_SCAN): n_kept = sites it holds, index_bytes = device memory it
 * takes (0 = the matrix has none; compacted matrices never have one, all their sites are kept); why (nullable, why_len
 * bytes) receives the reason there is none, or "" when there is one.  All outputs nullable. */
int impop_matrix_scan_index_info(const impop_matrix *m, uint64_t *n_kept, uint64_t *index_bytes, char *why, size_t why_len);
/* The rare/common split of that index (see IMPOP_KEEP_NO_RARE_SPLIT): n_rare = rare sites (8-byte entries), n_common = kept
 * sites stored as rows, rare_bytes = bytes of the entries; all 0 when there is no split, and why (nullable, why_len bytes)
 * receives the reason, else "".  All outputs nullable. */
int impop_matrix_scan_split_info(const impop_matrix *m, uint64_t *n_rare, uint64_t *n_common, uint64_t *rare_bytes, char *why,
                                 size_t why_len);
/* The singleton stream of that split (see IMPOP_KEEP_NO_SINGLE_STREAM): n_single = singleton sites (2 bytes each), n_multi = the
 * other rare sites (8-byte entries), stream_bytes = device memory the two streams and their per-block mask and prefix take
 * (counted in impop_matrix_scan_index_info's index_bytes); all 0 when there is none, and why (nullable, why_len bytes) receives
 * the reason, else "".  impop_matrix_scan_split_info reports what it did before: every rare site, 8 bytes each.  All outputs
 * nullable. */
int impop_matrix_scan_single_info(const impop_matrix *m, uint64_t *n_single, uint64_t *n_multi, uint64_t *stream_bytes, char *why,
                                  size_t why_len);
/* The distinct-row stream of that split (see IMPOP_KEEP_NO_UNIQUE_ROWS): n_unique = representatives over all 64-row blocks of
 * the common rows, n_common = those rows, stream_bytes = device memory of the representatives' rows, their weight bytes and the
 * per-block mask and prefix (counted in index_bytes); all 0 when there is none, and why receives the reason, else "".  All
 * outputs nullable. */
int impop_matrix_scan_unique_info(const impop_matrix *m, uint64_t *n_unique, uint64_t *n_common, uint64_t *stream_bytes, char *why,
                                  size_t why_len);
int impop_matrix_free(impop_ctx *ctx, impop_matrix *m);

/* ---- windowed scan: pi + Hudson Fst + Tajima's D + S in one pass ------------
 * Replaces, per window, the chain run_pica2_impg.sh:175 / run_h-fst.sh:74 /
 * run_tajd.sh:148,166,180, i.e. pica2.analyze_similarity_matrix (pica2.py:60)
 * at threshold >= 1 (every haplotype its own group), h-fst.calculate_fst
 * (h-fst.py:173) and tj_d.tajimas_d (tj_d.py:47) on the `match` identity
 * sim_ij = (W - H_ij)/W of the window's W sites, using the exact identities
 *   sum_{i<j in P} H_ij = sum_s c_P,s (n_P - c_P,s)
 *   sum_{i in A, j in B} H_ij = sum_s [c_A,s (n_B - c_B,s) + c_B,s (n_A - c_A,s)]
 * (SURVEY.md Appendix A.1), so one streaming pass over the bit matrix suffices.
 * n_hap <= 65535 for impop_scan_plan_create / impop_scan / impop_scan_multi / impop_scan_sharded (the per-site
 * products c (n - c) stay below 2^32); a matrix of more haplotypes is refused with IMPOP_E_INVALID. */
typedef struct impop_window {
    uint64_t site_begin;  /* first site of the window */
    uint64_t site_end;    /* one past the last site */
    uint64_t seq_len;     /* `-l` of pica2.py:177 / h-fst.py:278; 0 = not given */
} impop_window;

typedef struct impop_window_stats { /* 128 bytes, fixed layout */
    uint32_t n_sites;     /* W */
    uint32_t s_all;       /* #{s: 0 < c_s < n} over all rows (run_tajd.sh:126,148: un-subset graph) */
    uint32_t s_p;         /* segregating within subset P */
    uint32_t s_a, s_b;    /* segregating within A, within B */
    uint32_t flags;       /* reserved, 0 */
    uint64_t sum_p;       /* sum_s cP (nP - cP)      = sum_{i<j in P} H_ij */
    uint64_t sum_a;       /* sum_s cA (nA - cA) */
    uint64_t sum_b;       /* sum_s cB (nB - cB) */
    uint64_t sum_ab;      /* sum_s cA(nB-cB) + cB(nA-cA) = sum_{A x B} H_ij */
    double pi;            /* pica2.py:154  (mean over pairs in P of 1 - sim) */
    double pi_site;       /* pica2.py:164  pi / seq_len; NaN when seq_len == 0 (None) */
    double pi_a, pi_b, pi_xy, dxy, da; /* h-fst.py:233-249 (divided by seq_len when > 0) */
    double fst;           /* h-fst.py:214-221 */
    double tajima_d;      /* tj_d.py:47-69; NaN where the reference prints nan/NA */
} impop_window_stats;

typedef struct impop_scan_params {
    uint32_t struct_size; /* sizeof(impop_scan_params) */
    /* which pi feeds Tajima's D: 0 = as wired by run_tajd.sh:166-180 (per-site pi
     * through the "%.8f" text round trip), 1 = per-site pi unrounded,
     * 2 = mean pairwise differences pi*W (textbook; not what the reference does) */
    int32_t d_pi_mode;
    /* S used for D: 0 = all rows of the matrix (run_tajd.sh:126,148), 1 = within P */
    int32_t s_scope;
    uint32_t tile_blocks; /* 0 = default; 64-site blocks per work tile (tuning) */
} impop_scan_params;

/* Masks are n_hap-bit little-endian bitsets (uint64 words).  mask_p: the
 * sample subset for pi / D (run_tajd.sh -l list; NULL = all haplotypes);
 * mask_a / mask_b: populations for Hudson Fst (NULL = empty).  Haplotypes in
 * both A and B are removed from both (h-fst.py:181-185). */
int impop_scan_plan_create(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows,
                           const uint64_t *mask_p, const uint64_t *mask_a, const uint64_t *mask_b,
                           const impop_scan_params *params, impop_scan_plan **out);
/* Replace the three subset masks of an existing plan (the tile tables depend on the windows only), e.g.
 * to scan the same windows for many population pairs; takes effect for launches issued afterwards.
 * A launch captured into a graph BEFORE this call keeps the subset sizes and kernel choice it was
 * captured with: after impop_scan_plan_set_masks, capture again. */
int impop_scan_plan_set_masks(impop_scan_plan *plan, const uint64_t *mask_p, const uint64_t *mask_a,
                              const uint64_t *mask_b);
/* Enqueue one pass over all windows on the context's stream (no host sync, no
 * allocation: graph-capturable).  d_out: device buffer of n_windows records, or
 * NULL to use the plan's internal buffer.
 * A launch is two kernels on buffers the plan owns (its Tajima constants among them) and touches no
 * state of the context.  A captured launch is a snapshot of the plan's kernel choice and subset sizes;
 * any number of plans, and of graphs captured from them, may share a context and be launched, replayed
 * and mixed with every other call on it in any order. */
int impop_scan_plan_launch(impop_scan_plan *plan, void *d_out);
/* Synchronise and copy the plan's internal result buffer to the host. */
int impop_scan_plan_fetch(impop_scan_plan *plan, impop_window_stats *out_host);
/* bytes_streamed: layout bytes one launch reads (of the kept-site layout when the plan streams the scan index; where a tile
 * takes the distinct-row stream, the whole blocks of that stream its range touches and their 64 weight bytes each, in place
 * of the tile's whole blocks of rows).
 * Under IMPOP_TRACE=1 impop_scan_plan_create prints one line per plan on stderr:
 *   [impop_scan] route=<indexed|dense|compact> kept_sites=<n> tiles=<n> bytes_streamed=<n> windows=<n> rare_sites=<n>
 *                rare_bytes=<n> split=<on|off:reason> single_sites=<n> rare_streamed=<n> unique_rows=<n> rows_streamed=<n> wave_tiles=<0|1>
 *                digest=<0|1> [why=<reason>]
 * unique_rows: the representatives of the matrix's distinct-row stream when the plan reads it, else 0; rows_streamed: the bytes
 * of rows (and representatives) among bytes_streamed, rare_streamed the rest; wave_tiles: the plan's launches run one wave per
 * tile (small tiles in number; IMPOP_SCAN_WAVE_TILES=0|1 where the plan is made: never / whenever the 32-bit lane sums allow). */
int impop_scan_plan_info(const impop_scan_plan *plan, uint64_t *n_tiles, uint64_t *bytes_streamed);
/* The plan's tile digest (digest=1 of the trace line).  A plan and its matrix do not change, only the masks do, so a plan of
 * many small tiles that its maker will launch again works out once, per tile, what no mask enters: the tile's distinct common
 * rows under complement with a weight each, and how many of its singleton sites every haplotype carries.  Launches then read
 * the digest in place of the rows and the singleton stream, and bytes_streamed counts that.  Taken by default where the plan
 * runs one wave per tile, every tile fits the digest's caps and a launch reads no more bytes than without; never for the
 * one-shot impop_scan.  IMPOP_SCAN_DIGEST=0|1 where the plan is made: never / whenever the caps allow.  Records are the same
 * bytes either way.  on: 0|1; n_rows: representatives over all tiles; n_hist_tiles: tiles with a histogram; digest_bytes: device
 * memory the digest holds; why: the reason there is none, else "".  Every pointer may be NULL. */
int impop_scan_plan_digest_info(const impop_scan_plan *plan, int *on, uint64_t *n_rows, uint64_t *n_hist_tiles, uint64_t *digest_bytes,
                                char *why, size_t why_len);
/* Measurement aid: with timing enabled every launch brackets the streaming kernel
 * (not the tiny epilogue) with hipEvents on the context's stream; elapsed() synchronises
 * and returns the summed kernel time and the number of launches since enable/reset. */
int impop_scan_plan_timing(impop_scan_plan *plan, int enable);
int impop_scan_plan_elapsed(impop_scan_plan *plan, double *total_ms, uint64_t *launches);
int impop_scan_plan_destroy(impop_scan_plan *plan);
/* Convenience: create + launch + fetch + destroy. */
int impop_scan(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows,
               const uint64_t *mask_p, const uint64_t *mask_a, const uint64_t *mask_b,
               const impop_scan_params *params, impop_window_stats *out_host);

/* K disjoint populations, all K(K-1)/2 Hudson Fst pairs in ONE streaming pass: replaces the
 * panel loops of run_h_fst_panels.sh:60-71 (one run_h-fst.sh per population pair).
 * masks: n_pop bitsets of ceil(n_hap/64) uint64 words each; populations must be disjoint.
 * out: n_windows x K(K-1)/2 records, pairs ordered (0,1),(0,2),...,(1,2),...; per pair the six
 * values of h-fst.py:233-249 with population k as A and l as B. */
typedef struct impop_pair_stats {
    double fst, pi_a, pi_b, pi_xy, dxy, da;
} impop_pair_stats;
int impop_scan_multi(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows,
                     const uint64_t *masks, uint32_t n_pop, impop_pair_stats *out_host);

/* Allele-frequency spectrum per window (scripts/wip/op-afs.py): out[w*(nP+1) + c] = number of
 * sites of window w at which exactly c haplotypes of `mask` (NULL = all; nP = its size) carry the
 * allele.  nP <= 16383 (the nP + 1 bins of a window are one workgroup's 64 KiB LDS histogram); a larger
 * mask returns IMPOP_E_INVALID.  Any number of windows. */
int impop_afs(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows,
              const uint64_t *mask, uint32_t *out_host);

/* Per-site allele counts c_s of the haplotypes in `mask` (NULL = all) for sites
 * [site_begin, site_end): the per-site allele frequency is c_s / n. */
int impop_site_counts(impop_ctx *ctx, const impop_matrix *m, const uint64_t *mask, uint64_t site_begin,
                      uint64_t site_end, uint32_t *counts_out_host);

/* Extended haplotype homozygosity, calc_EHH of scripts/wip/ehhgfa.py:6-21: out[i] =
 * round(#{pairs of `mask` members (NULL = all) identical on window sites 0..i} / (m(m-1)/2), 3),
 * i over [site_begin, site_end).  reverse != 0 walks the window from its last site backwards
 * (calc_EHH of the column-flipped matrix, ehhgfa.py:61).  m < 2 fills 500.0 (ehhgfa.py:17-18).
 * n_members (nullable) receives m. */
int impop_ehh(impop_ctx *ctx, const impop_matrix *m, uint64_t site_begin, uint64_t site_end, const uint64_t *mask,
              int reverse, double *ehh_out_host, uint32_t *n_members);

/* Integrated EHH per core site for a batch of windows (the scan of scripts/wip/ehhgfa.py:40-69, which keeps only the
 * integral of each curve, :63).  Every (window, allele a, half h) is one calc_EHH problem: its members are the haplotypes
 * of P (mask_p, NULL = all) whose bit at core_site equals a, its sites and direction are
 *     flanks REFERENCE: half 0 = (core, end) walked backwards from end - 1, half 1 = (core, end) walked forwards
 *     flanks TWO_SIDED: half 0 = [begin, core) walked backwards from core - 1, half 1 = (core, end) walked forwards
 * and EHH[i] is exactly the double impop_ehh returns for that range, members and direction: k / 1000 for an integer k.
 * area_milli is the sum of those k over the half's sites - an integer, so no summation order enters and chunking never
 * changes a record - and area[a] = (area_milli[a][0] + area_milli[a][1]) / 1000.0.  A problem with one member counts
 * 500 000 per site (ehhgfa.py:17-18), one without members 0 (n_members 0), an empty flank 0.
 * |P| <= IMPOP_EHH_SCAN_MAX_N: a problem's class labels, representatives and sizes (12 bytes per member) stay in the LDS
 * of its workgroup; a larger |P| returns IMPOP_E_UNSUPPORTED (impop_ehh takes up to 65535 members).  A compacted matrix
 * returns IMPOP_E_UNSUPPORTED; a core outside its window, a window outside the matrix or ref_hap >= n_hap return
 * IMPOP_E_INVALID; all of these before anything is uploaded or launched.  Windows may overlap or repeat with other cores.
 * Two kernel launches per chunk of windows whatever their number (a chunk holds up to max_chunk_bytes of transposed
 * window words, at most 65535 windows); checks the device error word like impop_pairwise_scan. */
#define IMPOP_EHH_SCAN_MAX_N 4096u
typedef struct impop_ehh_window {
    uint64_t site_begin, site_end, core_site;  /* core in [begin, end) */
} impop_ehh_window;
#define IMPOP_EHH_FLANKS_REFERENCE 0 /* both halves from the right flank (core, end): ehhgfa.py:56-61 */
#define IMPOP_EHH_FLANKS_TWO_SIDED 1 /* half 0 = [begin, core) walking away from the core, half 1 = (core, end) */
typedef struct impop_ehh_params {
    uint32_t struct_size;
    int32_t flanks;           /* IMPOP_EHH_FLANKS_* */
    uint32_t ref_hap;         /* haplotype whose core allele is reported as ref_allele (ehhgfa.py:52) */
    uint32_t reserved;
    uint64_t max_chunk_bytes; /* 0 = default (1 GiB); tests use it to force several chunks */
} impop_ehh_params;
typedef struct impop_ehh_stats { /* 64 bytes, fixed layout */
    uint32_t n_members[2];       /* members of P carrying allele 0 / 1 at the core site */
    uint32_t ref_allele;         /* allele of haplotype ref_hap at the core; REF / ALT is the caller's label */
    uint32_t reserved;
    int64_t area_milli[2][2];    /* [allele][half]: sum over the half's sites of 1000 * EHH[i], exact */
    double area[2];              /* (area_milli[a][0] + area_milli[a][1]) / 1000.0 */
} impop_ehh_stats;
int impop_ehh_scan(impop_ctx *ctx, const impop_matrix *m, const impop_ehh_window *windows, uint64_t n_windows,
                   const uint64_t *mask_p, const impop_ehh_params *params, impop_ehh_stats *out_host);
/* With impop_ctx_gram_timing on, impop_ehh_scan brackets the kernels of every chunk: their summed time and the number
 * of chunks since enable / reset. */
int impop_ctx_ehh_elapsed(impop_ctx *ctx, double *total_ms, uint64_t *launches);

/* Device address of the plan's internal record buffer (n_windows x impop_window_stats, written by launches
 * with d_out == NULL): what a caller hands to impop_gather_records without owning any device memory itself. */
int impop_scan_plan_device_records(impop_scan_plan *plan, void **d_records);

/* ---- multi-GPU -----------------------------------------------------------------
 * Replaces the serial per-window loops of run_tajd.sh:103-196, run_h-fst.sh:155-190 and run_pica2_impg.sh:126-190
 * ACROSS GPUs: no statistic spans windows, so the window list is cut into contiguous ranges (the first
 * n % shards ranges hold one window more), each GPU keeps only the slab of sites its windows touch (sliding
 * windows: slabs overlap by the halo) and the only exchange is ONE all-gather of the 128-byte records. */

/* items [first, first + count) of shard `shard` out of n_shards */
int impop_shard_range(uint64_t n_items, int n_shards, int shard, uint64_t *first, uint64_t *count);
/* the windows of a shard and the site range [slab_begin, slab_end) they touch (all outputs nullable) */
int impop_shard_windows(const impop_window *windows, uint64_t n_windows, int n_shards, int shard, uint64_t *first_window,
                        uint64_t *n_shard_windows, uint64_t *slab_begin, uint64_t *slab_end);

/* One process driving n_ctx devices (or n_ctx contexts of one device).  slabs[k] lives on ctxs[k] and holds the
 * sites [slab_site_begin[k], slab_site_begin[k] + its n_site) of the chromosome — at least the range
 * impop_shard_windows reports for shard k.  `windows` are in chromosome coordinates.  Every context launches its
 * pass before any result is waited for; out_host receives n_windows records in the order of `windows`, byte for
 * byte what one context holding the whole matrix returns. */
int impop_scan_sharded(impop_ctx *const *ctxs, const impop_matrix *const *slabs, const uint64_t *slab_site_begin, int n_ctx,
                       const impop_window *windows, uint64_t n_windows, const uint64_t *mask_p, const uint64_t *mask_a,
                       const uint64_t *mask_b, const impop_scan_params *params, impop_window_stats *out_host);

/* One process per GPU: a communicator over RCCL (xGMI inside a node).  Rank 0 calls impop_comm_unique_id and
 * hands the 128 bytes to the other ranks by any out-of-band means (file, MPI, the launcher's store); then every
 * rank calls impop_comm_create with its context.  RCCL is loaded (dlopen librccl.so.1) by these two calls only. */
#define IMPOP_COMM_ID_BYTES 128
typedef struct impop_comm impop_comm;
int impop_comm_unique_id(void *id_out /* IMPOP_COMM_ID_BYTES */);
int impop_comm_create(impop_ctx *ctx, const void *unique_id, int world, int rank, impop_comm **out);
int impop_comm_destroy(impop_comm *comm);
/* ncclAllGather of bytes_per_rank bytes from every rank into d_all (world x bytes_per_rank, rank order); device
 * pointers; enqueued on the context's stream behind the scans that wrote d_local — no host synchronisation. */
int impop_gather(impop_comm *comm, const void *d_local, size_t bytes_per_rank, void *d_all);
/* The scan's exchange step in one call: this rank's records (device pointer, the shard impop_shard_range gives
 * this rank out of n_total_windows; e.g. impop_scan_plan_device_records) are all-gathered and every rank
 * receives all n_total_windows records in global window order on the host.  Synchronises the stream. */
int impop_gather_records(impop_comm *comm, const void *d_local_records, uint64_t n_total_windows,
                         impop_window_stats *out_host);
/* The one reduction of the path: a single giant window's Gram matrix, site axis split over
 * ranks — in-place ncclAllReduce(sum) of `count` int64 on the device, on the context's stream. */
int impop_allreduce_i64(impop_comm *comm, int64_t *d_values, size_t count);

/* ---- all-pairs path -------------------------------------------------------
 * I_ij = #sites of the window carried by both i and j (the quantity behind
 * `impg similarity`'s estimated.identity, run_pica2_impg.sh:162); a_i = I_ii.
 * out: int32 [n_hap * n_hap] row-major on the host. */
int impop_pairwise_counts(impop_ctx *ctx, const impop_matrix *m, uint64_t site_begin, uint64_t site_end,
                          int32_t *out_host);

#define IMPOP_IDENTITY_MATCH 0 /* (W - H_ij)/W, H = a_i + a_j - 2 I_ij */
#define IMPOP_IDENTITY_DICE 1  /* 2 I_ij / (a_i + a_j); 0/0 -> 1.0 */

/* Identity matrix of a window as doubles (what a .sim file would hold). */
int impop_pairwise_identity(impop_ctx *ctx, const impop_matrix *m, uint64_t site_begin, uint64_t site_end,
                            int identity_kind, double *out_host);

/* Full pica2 / h-fst semantics (thresholds, rounding, grouping) for a batch of windows straight from the bit
 * matrix; identity never leaves the GPU.  af.py's clustering of the same windows is impop_cluster_scan below. */
typedef struct impop_pairwise_params {
    uint32_t struct_size;
    int32_t identity_kind;   /* IMPOP_IDENTITY_* */
    double threshold;        /* pica2 -t (pica2.py:175) */
    int32_t round_digits;    /* pica2 -r / h-fst -r; < 0 = none */
    int32_t d_pi_mode;       /* as impop_scan_params */
    int32_t s_scope;         /* as impop_scan_params; 2 = S and Tajima's D not needed: skips the site scan (s_all = s_p = 0, tajima_d = NaN) */
    uint32_t fst_method;     /* 0 = h-fst.py / hud.py direct; 1 = hud.py -m grouped at `threshold` (hud.py:64-128, 235-263) */
} impop_pairwise_params;
typedef struct impop_pairwise_stats { /* 96 bytes */
    double pi, pi_site;                      /* pica2.py:154,164 on subset P with grouping */
    double fst, pi_a, pi_b, pi_xy, dxy, da;  /* h-fst.py:233-249 */
    double tajima_d;                         /* tj_d.py:47 wired per d_pi_mode / s_scope */
    uint32_t n_groups;                       /* pica2.py:114 */
    uint32_t s_all, s_p, n_sites;
    uint64_t reserved;
} impop_pairwise_stats;
int impop_pairwise_scan(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows,
                        const uint64_t *mask_p, const uint64_t *mask_a, const uint64_t *mask_b,
                        const impop_pairwise_params *params, impop_pairwise_stats *out_host);
/* K disjoint panels and all their K(K-1)/2 pairs from ONE Gram pass per window: replaces the panel loops of
 * run_tajd_panels.sh:60-84 (run_tajd.sh per panel: pica2 -t 0.999 -r 5 on the panel's subset, then tj_d) and
 * run_h_fst_panels.sh:60-95 (run_h-fst.sh per pair) at ANY threshold, rounding and identity — where impop_scan_multi is exact
 * only for the direct method on unrounded `match`.  The Gram matrix of a window does not depend on the masks, so the K
 * impop_pairwise_scan(mask_p = panel k) and K(K-1)/2 impop_pairwise_scan(mask_a, mask_b) calls this replaces contract it
 * K + K(K-1)/2 times; here it is contracted once and the masks only select what the statistics kernels read.
 * masks: as impop_scan_multi — n_pop (2..8) bitsets of ceil(n_hap/64) uint64 words each, pairwise disjoint, none empty (anything
 * else: IMPOP_E_INVALID); haplotypes in no panel contribute nothing.
 * params: identity_kind, threshold, round_digits, d_pi_mode as impop_pairwise_scan; s_scope 0: S = s_all of the window from the
 * matrix's site bitmap; 1: S = s_p of the panel, from the streaming scan of the same windows with mask_p = the panel (one more
 * streaming pass per panel); 2: no S, tajima_d = NaN.  fst_method 1 returns IMPOP_E_UNSUPPORTED.
 * out_panels: n_windows x n_pop, a panel record equal byte for byte to the fields of the same name impop_pairwise_scan(mask_p =
 * the panel) returns (s_p: s_scope 1 only, else 0).  out_pairs (nullable: no Fst work is done): n_windows x K(K-1)/2 in the pair
 * order of impop_scan_multi, population k as A and l as B.  out_windows (nullable): n_sites, and s_all unless s_scope is 2.
 * Compacted and weighted matrices, overlapping windows and chunking as impop_pairwise_scan; records do not depend on any of
 * them, and two calls return identical bytes (the sums have one fixed order; no floating-point atomics).  Checks the device
 * error word like impop_pairwise_scan.  With impop_ctx_gram_timing on, impop_ctx_cluster_elapsed returns the summed time of the
 * chunks' Fst kernel(s) next to the Gram time.  Under IMPOP_TRACE=1 one line per call on stderr, next to the [impop_gram] lines:
 *   [impop_pairwise_scan_panel] pops=<K> pairs=<K(K-1)/2> route=<small|general>
 * small = one kernel reads the panels' union once for all pairs (n_hap <= 512, `match`, windows lighter than 2^30); general =
 * one h-fst launch per pair on the one Gram pass. */
typedef struct impop_panel_stats {      /* 48 bytes, fixed layout: one per (window, panel) */
    double pi, pi_site;                 /* pica2.py:154,164 on the panel's members, grouped at `threshold` */
    double tajima_d;                    /* tj_d.py:47 wired per d_pi_mode / s_scope, n = panel size */
    uint32_t n_members, n_groups, s_p, reserved;
    uint64_t reserved2;                 /* 0; pads the record to the 48 bytes of impop_pair_stats */
} impop_panel_stats;
typedef struct impop_panel_window { uint32_t n_sites, s_all; } impop_panel_window;   /* one per window */
int impop_pairwise_scan_panel(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows,
                              const uint64_t *masks, uint32_t n_pop, const impop_pairwise_params *params,
                              impop_panel_stats *out_panels, impop_pair_stats *out_pairs, impop_panel_window *out_windows);
#define IMPOP_CLUSTER_MAX_N 12798u /* see impop_cluster_from_identity */
/* af.cluster (af.py:35-54) for a batch of windows straight from the bit matrix: per window the connected components of
 * {identity(i, j) >= threshold} over the members of P, the identity being exactly the double impop_pairwise_identity
 * yields for that window (weights and compacted matrices included; rounded like pica2 -r when round_digits >= 0).
 * Clusters are ordered by (-size, smallest member index), as impop_cluster_from_identity orders them.  At threshold
 * 1.0 (af.py:73) the clusters are the window's distinct haplotypes: sizes is the haplotype frequency spectrum and
 * sum_sq / n_members^2 the haplotype homozygosity.
 * |P| <= IMPOP_CLUSTER_MAX_N; a larger |P| returns IMPOP_E_INVALID before anything is uploaded or launched.  A window
 * without sites has identity 1.0 for every pair (one cluster).  Checks the device error word like impop_pairwise_scan;
 * chunking never changes a record. */
typedef struct impop_cluster_params {
    uint32_t struct_size;
    int32_t identity_kind;   /* IMPOP_IDENTITY_MATCH / _DICE */
    double threshold;        /* af.py --threshold; linked when identity >= threshold (af.py:38) */
    int32_t round_digits;    /* < 0 = none (af.py does not round); >= 0: the identity pica2 -r would see */
    uint32_t reserved;
} impop_cluster_params;
typedef struct impop_cluster_stats { /* 32 bytes, fixed layout */
    uint32_t n_members;      /* |P| */
    uint32_t n_clusters;
    uint32_t largest;        /* size of c1 */
    uint32_t n_singletons;
    uint64_t sum_sq;         /* sum of size_k^2; haplotype homozygosity = sum_sq / n_members^2 */
    uint32_t n_sites, reserved;
} impop_cluster_stats;
/* cluster_of (nullable): n_windows x |P|, the 0-based cluster rank of each member of P in ascending haplotype index;
 * sizes (nullable): n_windows x |P|, first n_clusters valid, the rest 0. */
int impop_cluster_scan(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows,
                       const uint64_t *mask_p, const impop_cluster_params *params, impop_cluster_stats *out_host,
                       uint32_t *cluster_of, uint32_t *sizes);
#define IMPOP_PAIRDIST_MAX_N 4096u    /* members of the panels' union */
#define IMPOP_PAIRDIST_MAX_BINS 1024u
/* Pairwise-distance DISTRIBUTIONS per window, from the Gram pass of impop_pairwise_scan_panel: the mismatch distribution inside
 * each panel, the extremes between panels (d_min, G_min of Geneva et al. 2015, RND_min) with the haplotype pair that attains
 * them, and Hudson's nearest-neighbour statistic S_nn with its directional counts.  Exact integers throughout.
 * The distance of haplotypes i and j in a window is H_ij = sum_s w_s [b_is != b_js] = a_i + a_j - 2 I_ij, the weighted Hamming
 * distance (w_s = 1 on unweighted matrices); the per-window constant of a compacted matrix cancels.  No identity kind, no
 * threshold, no rounding.
 * masks: as impop_scan_multi — n_pop (1..8) bitsets of ceil(n_hap/64) uint64 words each, pairwise disjoint, none empty (anything
 * else: IMPOP_E_INVALID); haplotypes in no panel contribute nothing.  The union may hold at most IMPOP_PAIRDIST_MAX_N members: a
 * larger one returns IMPOP_E_UNSUPPORTED before anything is uploaded or launched.
 * out_panels: n_windows x n_pop, over the pairs i < j of the panel.  out_pairs (nullable; NULL when n_pop == 1): n_windows x
 * K(K-1)/2 in the pair order of impop_scan_multi, over i in panel k, j in panel l (k < l).  min_i .. max_j are haplotype indexes
 * of the matrix; among pairs that tie, the pair with the smallest i wins, then the smallest j (i from panel k in a pair record).
 * With n_pairs = 0: min_h = max_h = 0 and the four indexes are 0xFFFFFFFF.
 * Nearest neighbours of a pair record, for every member i of k u l:  d_i = min over j in (k u l) \ {i} of H_ij,  tied_i =
 * #{j : H_ij = d_i},  same_i = the number of those j in i's own panel.  nn_same_a / nn_same_b count the members of k / of l with
 * same_i = tied_i, nn_other_a / nn_other_b those with same_i = 0, and
 *     snn  = (sum_i (double)same_i / (double)tied_i) / (double)(m_k + m_l)
 * the sum running sequentially, from 0.0, over i in ascending haplotype index (plain left-to-right double additions);
 *     gmin = (double)min_h / ((double)sum_h / (double)n_pairs),   NaN when sum_h = 0.
 * Histograms (hist_bins B = 0: none, else 1..IMPOP_PAIRDIST_MAX_BINS; hist_width >= 1; both tables nullable): hist_within is
 * uint32 n_windows x n_pop x B, hist_between n_windows x K(K-1)/2 x B; a pair counts in bin min(H_ij / hist_width, B - 1), so
 * the last bin collects the overflow.
 * sum_h2 is exact when W_max^2 * P_max <= 2^64 - 1 (W_max: the largest W of the call's windows, P_max: the largest n_pairs of
 * any record); otherwise the call returns IMPOP_E_UNSUPPORTED before any launch and the message names both numbers.  Every other
 * sum fits whatever the input (H <= W <= 2^31, at most 2^23 pairs).
 * A window without sites has H = 0 for every pair; n_windows == 0 returns IMPOP_OK; windows may overlap.  Chunking
 * (IMPOP_PAIRWISE_CHUNK), uint16 or int32 Gram counts, the Gram chain length, compaction and weights never change a byte, and two
 * calls return identical bytes (integer atomics only; the one double sum has a fixed order).  Checks the device error word like
 * impop_pairwise_scan.  With impop_ctx_gram_timing on, impop_ctx_pairdist_elapsed returns the summed time of the chunks'
 * distribution kernel next to the Gram time.  Histograms are tallied in LDS where all (K + pairs) x B counters fit next to the
 * kernel's tables, else straight into the tables in global memory; IMPOP_PAIRDIST_LDS_BINS=n (0..36864, a test aid) lowers the
 * number of counters the LDS form takes.  Under IMPOP_TRACE=1 one line per call on stderr, next to the [impop_gram] lines:
 *   [impop_pairdist_scan] pops= pairs= members= windows= chunks= launches= hist_bins= hist=<off|lds|global>
 * Known answer: haplotypes 0000, 0001, 0111, 0001 over one 4-site window, panels {0,1} and {2,3}: H01 = 1, H02 = 3, H03 = 1,
 * H12 = 2, H13 = 0, H23 = 2.  Panel records: (n_pairs 1, sum_h 1, sum_h2 1, n_zero 0, min = max = 1 at (0,1)) and (1, 2, 4, 0,
 * min = max = 2 at (2,3)).  Pair record: n_pairs 4, sum_h 6, sum_h2 14, n_zero 1, min_h 0 at (1,3), max_h 3 at (0,2); (same,
 * tied) per member = (1,2), (0,1), (1,2), (0,1), so nn_same_a = nn_same_b = 0, nn_other_a = nn_other_b = 1, snn = 0.25,
 * gmin = 0.0. */
typedef struct impop_pairdist_params {
    uint32_t struct_size;
    uint32_t hist_bins;      /* 0 = no histograms */
    uint32_t hist_width;     /* >= 1, also when hist_bins is 0 */
    uint32_t reserved;
} impop_pairdist_params;
typedef struct impop_dist_panel {       /* 64 bytes, fixed layout: one per (window, panel) */
    uint32_t n_members;                 /* size of the panel */
    uint32_t n_sites;                   /* the window's W */
    uint64_t n_pairs;                   /* m (m - 1) / 2 */
    uint64_t sum_h, sum_h2, n_zero;     /* sum of H, of H^2, #{H = 0} */
    uint32_t min_h, max_h;
    uint32_t min_i, min_j, max_i, max_j;
} impop_dist_panel;
typedef struct impop_dist_pair {        /* 96 bytes, fixed layout: one per (window, pair k < l) */
    uint64_t n_pairs;                   /* m_k m_l */
    uint64_t sum_h, sum_h2, n_zero;
    uint32_t min_h, max_h;
    uint32_t min_i, min_j, max_i, max_j;
    uint32_t nn_same_a, nn_same_b, nn_other_a, nn_other_b;
    double snn, gmin;
    uint64_t reserved;                  /* 0 */
} impop_dist_pair;
int impop_pairdist_scan(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows,
                        const uint64_t *masks, uint32_t n_pop, const impop_pairdist_params *params,
                        impop_dist_panel *out_panels, impop_dist_pair *out_pairs /* nullable */,
                        uint32_t *hist_within /* nullable */, uint32_t *hist_between /* nullable */);
#define IMPOP_PCA_MAX_N 1024u   /* members of the mask */
#define IMPOP_PCA_MAX_K 8u
/* PRINCIPAL COMPONENTS per window ("local PCA", Li & Ralph 2019): the k largest eigenpairs of the double-centred distance matrix
 * of the members of one mask, from the Gram pass of impop_pairwise_scan.  For 0/1 haplotypes the Hamming distance is the squared
 * Euclidean distance, so B below is X X^T with X the haplotype matrix centred per site: its eigenvectors are the principal
 * component scores of the haplotypes.
 * Per window, over the members P of mask_p (m = |P|, ascending haplotype index; NULL = all haplotypes):
 *   H_ij  = the weighted Hamming distance of impop_pairdist_scan, a_i + a_j - 2 I_ij (polarity-invariant; the constant of a
 *           compacted matrix cancels),
 *   r_i   = sum_{j in P} H_ij,   t = sum_i r_i,   sum_h = sum_{i<j} H_ij = t / 2,
 *   B_ij  = -1/2 (H_ij - r_i/m - r_j/m + t/m^2);   as exact integers  2 m^2 B_ij = m (r_i + r_j) - m^2 H_ij - t.
 * trace(B) = sum_h / m,  B 1 = 0,  B is positive semidefinite with rank <= min(m - 1, number of sites).
 * Output: the k (1 .. IMPOP_PCA_MAX_K) largest eigenpairs (lambda_j, v_j) of B.  lambda is descending; each v_j is a unit 2-norm
 * vector of m doubles, orthogonal to the ones vector; sign: the component of largest magnitude is positive, the lowest index on
 * exact ties.  The proportion of variance explained by pair j is lambda_j m / sum_h.
 * Zero eigenvalues: a Ritz value theta_j <= tol trace(B) is reported as lambda_j = 0.0 with an all-zero vector; `rank` counts the
 * others (a prefix of the k).  A window with sum_h = 0 (no sites, or all members identical) has rank 0 and iterations 0.
 * Method and convergence: block subspace iteration with Rayleigh-Ritz on a block of 16 vectors (>= k + 8 for every k), in fp64.
 * It iterates until every j < rank has || B v_j - theta_j v_j ||_2 <= tol theta_1; if max_iter steps do not get there, flag bit 0
 * is set and the last iterate and its residuals are returned (the call still returns IMPOP_OK).  Guaranteed regime: with the
 * default max_iter = 500 a window converges whenever lambda_{k+9} <= 0.9 lambda_j for every non-zero lambda_j, j <= k, of the
 * exact spectrum (a block of at least k + 8 vectors contracts the error of pair j by at most lambda_{k+9} / lambda_j per step, and
 * 0.9^500 ~ 1e-23).  Outside it, raise max_iter or read the flag.
 * Determinism: the start block is a fixed function of (member position, column); every reduction has one fixed order and there
 * are no floating-point atomics; everything the solver reads is an exact integer.  Two calls return identical bytes, and none of
 * chunking (IMPOP_PAIRWISE_CHUNK), uint16 or int32 Gram counts (IMPOP_GRAM_U16=0), the Gram chain length (IMPOP_GRAM_CHAIN),
 * compaction, weights against the bp-expanded matrix, or the order of the windows in the list changes a byte of a window's result.
 * out_windows: n_windows records.  out_vectors (nullable): n_windows x k x |P| doubles, vector j of window w at (w k + j) |P|.
 * out_dist2 (nullable): n_windows x n_windows, lostruct's distance between windows: with a_j = lambda_j / sum_{i<k} lambda_i,
 *   d2(w, w') = sum_j a_j^2 + sum_l a'_l^2 - 2 sum_{j,l} a_j a'_l (v_j . v'_l)^2,
 * clamped at 0 from below; exactly symmetric, the diagonal exactly 0; rows and columns of windows with rank 0 or flag bit 0 are
 * NaN, the diagonal included.  d2 does not depend on the vectors' signs nor on rotations inside an eigenspace.  It is one launch
 * after the last chunk, over the vectors of all windows, which stay on the device for it.
 * Refusals, all before anything is uploaded or launched: struct_size mismatch, k = 0 or k > IMPOP_PCA_MAX_K, tol outside
 * [1e-13, 1e-2], max_iter outside 1 .. 100000, |P| < 2, out_dist2 without out_vectors: IMPOP_E_INVALID; |P| > IMPOP_PCA_MAX_N,
 * out_dist2 with more than 16384 windows: IMPOP_E_UNSUPPORTED.  n_windows == 0 returns IMPOP_OK.  Windows may overlap; a
 * weighted matrix gives what its bp-expanded matrix gives.  Checks the device error word like impop_pairwise_scan.  With
 * impop_ctx_gram_timing on, impop_ctx_pca_elapsed returns kernel_ms[0] = the eigen kernel of every chunk, [1] = the distance
 * kernel, summed since enable / reset, next to the Gram time; chunks = eigen launches timed.
 * Under IMPOP_TRACE=1 one line per call on stderr, next to the [impop_gram] lines:
 *   [impop_pca_scan] route=<dense|compact> members= k= windows= chunks= launches= iterations_max= unconverged= dist=<off|on>
 * Known answer: haplotypes 0000, 0001, 0111, 0001 over one 4-site window, all members: H01 = 1, H02 = 3, H03 = 1, H12 = 2,
 * H13 = 0, H23 = 2; r = (5, 3, 7, 3), t = 18, sum_h = 9, trace = 2.25;
 * 32 B = [[22, -2, -18, -2], [-2, 6, -10, 6], [-18, -10, 38, -10], [-2, 6, -10, 6]];
 * lambda = (9 +- sqrt(17)) / 8 = 1.6403882032022..., 0.6096117967977..., the rest 0;
 * v_1 = (-0.472668, -0.184524, 0.841716, -0.184524). */
typedef struct impop_pca_params {   /* 24 bytes */
    uint32_t struct_size, k;
    double tol;                     /* relative residual bound, 1e-13 <= tol <= 1e-2; the Python and CLI default is 1e-10 */
    uint32_t max_iter, reserved;    /* 1 .. 100000; default 500 */
} impop_pca_params;
typedef struct impop_pca_window {   /* 160 bytes, fixed layout: one per window */
    uint32_t n_members, n_sites;
    uint32_t rank;                  /* eigenvalues reported non-zero, <= k */
    uint32_t iterations;
    uint32_t flags;                 /* bit 0: not converged within max_iter */
    uint32_t reserved;
    uint64_t sum_h;                 /* exact; trace(B) = sum_h / n_members */
    double lambda[8];               /* descending; 0.0 for rank <= j < k; NaN for j >= k */
    double resid[8];                /* ||B v_j - lambda_j v_j||_2 as last evaluated; NaN for j >= rank */
} impop_pca_window;
int impop_pca_scan(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows,
                   const uint64_t *mask_p /* nullable */, const impop_pca_params *params, impop_pca_window *out_windows,
                   double *out_vectors /* nullable: n_windows x k x |P| */, double *out_dist2 /* nullable: n_windows x n_windows */);
#define IMPOP_TREE_MAX_N 1024u   /* members of the mask */
enum { IMPOP_LINKAGE_SINGLE = 0, IMPOP_LINKAGE_COMPLETE = 1, IMPOP_LINKAGE_AVERAGE = 2 };
/* LINKAGE TREES per window ("local trees"): the single-, complete- or average-linkage (UPGMA) tree of the members of one mask over
 * their Hamming distances, from the Gram pass of impop_pairwise_scan, and per panel where it forms a clade.  Exact integers
 * throughout, with one fixed tie rule: the output is a function of the distances alone.
 * Members and distances: the members P of mask_p (NULL = all haplotypes) are positions 0 .. m - 1 in ascending haplotype index,
 * m = |P| >= 2.  H_ij is the weighted Hamming distance of impop_pairdist_scan, a_i + a_j - 2 I_ij (polarity-invariant; the constant
 * of a compacted matrix cancels).
 * Clusters and values: every member starts as a cluster NAMED by its position.  The value of a pair of live clusters (A, B) is
 *   single: min H_ij,   complete: max H_ij,   average: S_AB / (|A| |B|) with S_AB = sum H_ij,   over i in A, j in B.
 * Merge rule: each of the m - 1 steps merges the live pair with the smallest (value, a, b), lexicographic, a < b the clusters'
 * names (a cluster's name is its lowest member position).  Average linkage compares values EXACTLY, S_1 D_2 against S_2 D_1 as full
 * 128-bit products: S <= W D with W < 2^31 and D = |A| |B| <= 2^18, and two pairs live at once have D_1 D_2 <= m^4 / 64 = 2^34
 * (|A|^2 |B| |C| with |A| + |B| + |C| <= m = 1024, largest at |A| = m / 2), so a product reaches 2^65: 64 bits do not hold it.
 * The merged cluster keeps the name a; its distances follow Lance-Williams in integers: the min, the max, or the sum of the two sums.
 * out_merges (nullable): n_windows x (m - 1) records in merge order.  num is the value's numerator; the denominator is
 * size_a size_b for average linkage and 1 otherwise.  All three linkages are reducible (d(K, A u B) >= min(d(K, A), d(K, B))), so
 * the values are non-decreasing in merge order.  n_zero_merges counts the merges at value 0 (m minus the distinct haplotypes of the
 * window); n_tied_merges counts the steps at which at least two live pairs attain the minimum: there the topology is the tie
 * rule's.  root_num, root_size_a, root_size_b repeat the last merge.
 * Panels (n_pop 0..8; out_panels n_windows x n_pop, required exactly when n_pop > 0): panel_masks are n_pop bitsets as in
 * impop_pairdist_scan, disjoint and non-empty, and subsets of P (a panel member outside mask_p: IMPOP_E_INVALID).  largest_clade is
 * the size of the largest cluster ever formed, singletons included, whose members all lie in the panel.  mrca_size is the size of
 * the first cluster that holds the whole panel, mrca_merge the index of that merge (0xFFFFFFFF for a one-member panel, whose
 * mrca_size is 1): the panel is monophyletic IN THE TREE AS OUTPUT iff mrca_size == n_members.  Members in no panel count towards
 * sizes only.
 * Refusals, all before anything is uploaded or launched: struct_size mismatch, linkage > 2, |P| < 2, n_pop > 8, out_panels given
 * without n_pop or n_pop without out_panels, panels that overlap, are empty or leave P: IMPOP_E_INVALID; |P| > IMPOP_TREE_MAX_N:
 * IMPOP_E_UNSUPPORTED.  n_windows == 0 returns IMPOP_OK.
 * A window without sites has every value 0: m - 1 zero merges (0, 1), (0, 2), ..., all tied except the last, when only one pair is
 * left.  Windows may overlap.  None of chunking (IMPOP_PAIRWISE_CHUNK), uint16 or int32 Gram counts (IMPOP_GRAM_U16=0), the Gram
 * chain length (IMPOP_GRAM_CHAIN), compaction, weights against the bp-expanded matrix, the order of the windows in the list, or the
 * width in which the kernel stores its sums (uint32 where W floor(m^2 / 4) < 2^32 proves they fit, else uint64; IMPOP_TREE_WIDE=1,
 * a test aid, forces uint64) ever changes a byte, and two calls return identical bytes.  Checks the device error word like
 * impop_pairwise_scan.  With impop_ctx_gram_timing on, impop_ctx_tree_elapsed returns the summed time of the chunks' tree kernel
 * next to the Gram time.
 * The kernel never rescans the matrix per step: every live row caches its nearest neighbour, and a merge rescans only row a and
 * the rows whose cached neighbour was a or b.  Under IMPOP_TRACE=1 one line per call on stderr, next to the [impop_gram] lines:
 *   [impop_tree_scan] route=<dense|compact> linkage=<single|complete|average> members= pops= windows= chunks= launches=
 *                     rows_recomputed= tied_windows=
 * rows_recomputed sums, over all merges of the call, the live rows whose cached neighbour was a or b — a and b themselves among
 * them, so it is at least 2 (m - 1) per window; b retires, the others are rescanned.  tied_windows: windows with n_tied_merges > 0.
 * Known answer: haplotypes 0000, 0001, 0111, 0001 over one 4-site window, all members: H01 = 1, H02 = 3, H03 = 1, H12 = 2,
 * H13 = 0, H23 = 2.  Average linkage, merges (a, b, size_a, size_b, num): (1, 3, 1, 1, 0); then S_01 = H01 + H03 = 2 over 2 pairs
 * = 1 against S_12 = 4 over 2 = 2 and H02 = 3: (0, 1, 1, 2, 2); then (0, 2, 3, 1, 7), value 7/3.  n_zero_merges 1, n_tied_merges 0,
 * sum_h 9, root (7, 3, 1).  Panels {0, 1} and {2, 3}: largest_clade 1 / 1, mrca_size 3 / 4, mrca_merge 1 / 2.  Single linkage:
 * (1, 3, 1, 1, 0), (0, 1, 1, 2, 1), (0, 2, 3, 1, 2).  Complete linkage: (1, 3, 1, 1, 0), (0, 1, 1, 2, 1), (0, 2, 3, 1, 3). */
typedef struct impop_tree_params {   /* 8 bytes */
    uint32_t struct_size, linkage;   /* IMPOP_LINKAGE_* */
} impop_tree_params;
typedef struct impop_tree_window {   /* 48 bytes, fixed layout: one per window */
    uint32_t n_members, n_sites;
    uint32_t n_zero_merges;          /* merges at value 0: n_members - (distinct haplotypes of the window) */
    uint32_t n_tied_merges;          /* merges whose value another live pair equalled: the topology there is the tie rule's */
    uint64_t sum_h;                  /* as impop_pca_window.sum_h */
    uint64_t root_num;               /* the last merge */
    uint32_t root_size_a, root_size_b;
    uint64_t reserved;               /* 0 */
} impop_tree_window;
typedef struct impop_tree_merge {    /* 24 bytes: n_members - 1 per window, in merge order */
    uint32_t a, b;                   /* a < b: member POSITIONS naming the two clusters */
    uint32_t size_a, size_b;
    uint64_t num;                    /* single: min, complete: max, average: SUM of H_ij over i in A, j in B */
} impop_tree_merge;
typedef struct impop_tree_panel {    /* 16 bytes: one per (window, panel) */
    uint32_t n_members, largest_clade, mrca_size, mrca_merge;
} impop_tree_panel;
int impop_tree_scan(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows,
                    const uint64_t *mask_p /* nullable = all */, const uint64_t *panel_masks /* nullable */, uint32_t n_pop /* 0..8 */,
                    const impop_tree_params *params, impop_tree_window *out_windows, impop_tree_merge *out_merges /* nullable */,
                    impop_tree_panel *out_panels /* nullable; required non-NULL iff n_pop > 0 */);
#define IMPOP_PERMTEST_MAX_N 1024u      /* members of the panels' union */
#define IMPOP_PERMTEST_MAX_PERM 16384u  /* labellings of a call */
/* PERMUTATION P-VALUES for Hudson's Fst, AMOVA Phi_ST, Dxy and Hudson's S_nn (Hudson 2000) per window and pair of panels, from
 * the Gram pass of impop_pairdist_scan.  The device adds integers only.
 * masks, n_pop: as impop_pairdist_scan — disjoint, non-empty bitsets — with n_pop 2..8 and at most IMPOP_PERMTEST_MAX_N members in
 * the union of all panels.  out_pairs: n_windows x K(K-1)/2 records in the pair order of impop_scan_multi.
 * For a pair k < l: U = the members of k u l in ascending haplotype index, positions 0 .. m - 1 (m = m_k + m_l).  A LABELLING z is
 * an m-bit mask (bit i of word i / 64) with exactly m_k ones; z0, the observed labelling, marks the members of k.
 * Integers of a labelling, with H_ij the weighted Hamming distance of impop_pairdist_scan (polarity, compaction and weights cancel
 * as they do there):
 *   wa(z) = sum_{i<j, z_i=z_j=1} H_ij,   wb(z) = sum_{i<j, z_i=z_j=0} H_ij,   tot = sum_{i<j in U} H_ij,   ab(z) = tot - wa - wb.
 * Nearest neighbours do not depend on the labelling: d_i = min_{j != i in U} H_ij, T_i = {j : H_ij = d_i}, tied_i = |T_i|; then
 *   same_i(z) = #{j in T_i : z_j = z_i},   nn(z) = sum_i same_i(z) * floor(SCALE / tied_i),   SCALE = 2952069120 (= 720720 * 4096).
 * SCALE makes equal multisets of terms sum to equal integers in any order; the sum is exact whenever tied_i <= 16 or tied_i divides
 * SCALE.
 * "At least as extreme": all four tests are one-sided, towards more differentiation, and compared in integers:
 *   dxy:  ab(z) >= ab(z0)
 *   phi:  wa(z) m_l + wb(z) m_k <= wa(z0) m_l + wb(z0) m_k   (AMOVA Phi_ST of two groups, Excoffier et al. 1992: Phi_ST falls
 *         strictly as the within-group SSD rises, because the total SSD is fixed)
 *   fst:  x(z) ab(z0) <= x(z0) ab(z) as 128-bit products, x(z) = wa q_l + wb q_k, q = max(m (m - 1) / 2, 1) of the panel (Hudson,
 *         the estimator of h-fst.py).  The inequality is the definition in the degenerate cases too: ab(z) = 0 with x(z) > 0 is
 *         not counted against a z0 with ab(z0) > 0; tot = 0 counts every labelling.
 *   snn:  nn(z) >= nn(z0)
 * Labellings.  impop_permtest_labels is the one definition: labelling r of pair index p is a uniform random m_k-subset of the m
 * positions, a function of (seed, p, m, m_k, r) only — not of n_perm, the windows, the chunking or the device — so a call with fewer
 * permutations sees a prefix.  Generator: sm(x) = splitmix64's output for state x, that is z = x + 0x9E3779B97F4A7C15;
 * z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; return z ^ (z >> 31).  k1 = sm(seed),
 * k2 = sm(k1 ^ p), k3 = sm(k2 ^ r), u_t = sm(k3 + t * 0x9E3779B97F4A7C15) (all mod 2^64).  A partial Fisher-Yates over
 * a[0 .. m) = 0 .. m - 1: step t = 0 .. m_k - 1 swaps a[t] with a[t + hi], hi = the high 64 bits of the 128-bit product
 * u_t * (m - t); the labelling's ones are a[0 .. m_k).  The same labellings serve every window of a call (the tables are built once,
 * on the host, and uploaded): THE P-VALUES OF NEIGHBOURING WINDOWS THEREFORE SHARE THEIR NULL DRAWS.
 * Record: n_a = m_k, n_b = m_l, n_sites = the window's W; wa, wb, ab, nn of z0; ge_* = how many of the n_perm labellings are counted
 * above (z0 itself is not among them); p_* = (1.0 + (double)ge) / ((double)n_perm + 1.0).  The observed doubles are in raw distance
 * units, not divided by W (fst and phi_st are scale-free), finalised on the host from the integers in this order:
 *   dxy    = (double)ab / ((double)m_k * (double)m_l)
 *   pi_a   = (double)wa / (double)q_k when m_k >= 2, else 0.0; pi_b likewise from wb, q_l, m_l;  pi_xy = (pi_a + pi_b) / 2.0
 *   fst    = (dxy - pi_xy) / dxy when dxy > 0.0, else 0.0                                              
 *   phi_st = NaN when m <= 2; else ssd_w = (double)wa / (double)m_k + (double)wb / (double)m_l;  ssd_a = (double)tot / (double)m - ssd_w;
 *            ms_w = ssd_w / (double)(m - 2);  n0 = 2.0 * (double)m_k * (double)m_l / (double)m;  s2a = (ssd_a - ms_w) / n0;
 *            den = s2a + ms_w;  phi_st = s2a / den, NaN when den == 0.0
 *   snn    = the snn of impop_pairdist_scan for the same pair (same bytes): the left-to-right sum of (double)same_i(z0) /
 *            (double)tied_i over i ascending, divided by (double)m
 * out_null (nullable): n_windows x pairs x n_perm entries {wa, wb, nn}, the null distribution; allowed when n_windows * pairs *
 * n_perm <= 2^22, otherwise IMPOP_E_UNSUPPORTED.
 * Refusals, all before anything is uploaded or launched.  IMPOP_E_INVALID: struct_size mismatch, n_pop < 2 or > 8, n_perm = 0 or >
 * IMPOP_PERMTEST_MAX_PERM, overlapping or empty masks.  IMPOP_E_UNSUPPORTED: union > IMPOP_PERMTEST_MAX_N; the null-table bound;
 * W_max * P_max^2 > 2^62 (W_max the widest window weight, P_max the largest q of any panel), so that x fits 63 bits and the 128-bit
 * products cannot overflow — the message names both numbers.  n_windows == 0 returns IMPOP_OK.
 * Two calls return identical bytes, and none of chunking (IMPOP_PAIRWISE_CHUNK), uint16 or int32 Gram counts (IMPOP_GRAM_U16=0),
 * the Gram chain length (IMPOP_GRAM_CHAIN), compaction, weights against the bp-expanded matrix, or the order of the windows changes a
 * byte.  Checks the device error word like impop_pairwise_scan; in particular every labelling task recomputes z0 on the matrix
 * cores and the call fails (IMPOP_E_INTERNAL) if that differs from the direct sums.  With impop_ctx_gram_timing on,
 * impop_ctx_permtest_elapsed returns kernel_ms[0] = the preparation kernel, [1] = the labelling kernel, summed since enable / reset.
 * Under IMPOP_TRACE=1 one line per call on stderr, next to the [impop_gram] lines:
 *   [impop_permtest_scan] route=<dense|compact> pops= pairs= members= perms= planes= windows= chunks= launches= null=<off|on>
 * (planes = the bytes a distance of the call takes, 1..4).
 * Known answer: haplotypes 0000, 0001, 0111, 0001 over one 4-site window, panels {0,1} and {2,3}: H01 = 1, H02 = 3, H03 = 1,
 * H12 = 2, H13 = 0, H23 = 2, tot = 9.  Observed: wa 1, wb 2, ab 6; T = ({1,3}, {3}, {1,3}, {1}), same(z0) = (1, 0, 1, 0),
 * nn = SCALE, snn = 0.25.  The six possible labellings by their A positions give (wa, wb) = {0,1}: (1,2), {0,2}: (3,0),
 * {0,3}: (1,2), {1,2}: (2,1), {1,3}: (0,3), {2,3}: (2,1); ab = 6 for all of them. */
typedef struct impop_permtest_params {  /* 16 bytes */
    uint32_t struct_size;
    uint32_t n_perm;                    /* 1 .. IMPOP_PERMTEST_MAX_PERM */
    uint64_t seed;
} impop_permtest_params;
typedef struct impop_perm_pair {        /* 128 bytes, fixed layout: one per (window, pair k < l) */
    uint32_t n_a, n_b, n_sites, n_perm;
    uint64_t wa, wb, ab, nn;            /* observed */
    uint32_t ge_fst, ge_phi, ge_dxy, ge_snn;
    double fst, phi_st, dxy, snn;       /* observed */
    double p_fst, p_phi, p_dxy, p_snn;
} impop_perm_pair;
typedef struct impop_perm_null {        /* 24 bytes */
    uint64_t wa, wb, nn;
} impop_perm_null;
int impop_permtest_scan(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows,
                        const uint64_t *masks, uint32_t n_pop, const impop_permtest_params *params, impop_perm_pair *out_pairs,
                        impop_perm_null *out_null /* nullable */);
/* Host only, no context: labellings 0 .. n_perm - 1 of pair index pair_index over m positions with m_a ones (1 <= m_a < m <=
 * IMPOP_PERMTEST_MAX_N, n_perm <= IMPOP_PERMTEST_MAX_PERM; else IMPOP_E_INVALID).  out: n_perm x ceil(m / 64) words. */
int impop_permtest_labels(uint64_t seed, uint32_t pair_index, uint32_t m, uint32_t m_a, uint32_t n_perm, uint64_t *out);
#define IMPOP_KINSHIP_MAX_N 2048u        /* individuals of a genotype handle */
#define IMPOP_KINSHIP_MAX_WATCH 1024u    /* watched pairs of a call */
/* A PAIR OF INDIVIDUALS per window: the 3 x 3 joint genotype table and KING kinship of every pair of diploid individuals, from the
 * Gram pass of impop_pairwise_scan.  Exact integers throughout.
 * Genotype planes.  impop_genotypes_create pairs haplotypes into individuals as impop_diploid_scan does (pairs: h1, h2 per
 * individual) and builds, on the device and from the source's site-major rows alone (the source need not have kept its hap-major
 * copy), two bit planes per individual over the sites: H_i = h1 ^ h2 (heterozygous) and A_i = h1 & h2 (homozygous for the allele).
 * The handle holds them as a 2N-row operand of the Gram kernel — rows H_0 .. H_{N-1}, A_0 .. A_{N-1}, stored as given (no polarity
 * row), sites beyond n_site zero — and owns all its memory: the source may be freed afterwards.  Swapping h1 and h2 changes nothing.
 * A compacted source gives compacted planes over the same kept sites (positions and the bitmap of the dropped all-ones sites are
 * copied); a source with site weights returns IMPOP_E_UNSUPPORTED: a site is a column here.  An index >= n_hap, h1 == h2, a
 * haplotype in two pairs and n_ind < 2 return IMPOP_E_INVALID, n_ind > IMPOP_KINSHIP_MAX_N IMPOP_E_UNSUPPORTED, all before anything
 * is allocated.  impop_genotypes_info: n_site = the sites the planes hold (kept sites when compacted).  impop_genotypes_download:
 * 2N rows (H then A) of the plane sites [site_begin, site_end), bit s - site_begin of a row = site s, like impop_matrix_download.
 * The scan.  Per window and pair i < j, with g = 0 hom-ref, 1 het, 2 hom-alt, t[a][b] = the sites where g_i = a and g_j = b.  From
 * the Gram entries HH = |H_i & H_j|, HA = |H_i & A_j|, AH = |A_i & H_j|, AA = |A_i & A_j| and the diagonals het = |H|, alt = |A|:
 *     t11 = HH  t12 = HA  t21 = AH  t22 = AA  t10 = het_i - HH - HA  t01 = het_j - HH - AH  t20 = alt_i - AH - AA
 *     t02 = alt_j - HA - AA  t00 = W - (the other eight)
 * On compacted planes the window's dropped all-ones sites count in alt_i, alt_j and AA alone.  het_het = t11, ibs0 = t02 + t20,
 * ibs1 = t01 + t10 + t12 + t21, ibs2 = t00 + t11 + t22.  A cell that would come out negative sets the device error word: the call
 * returns IMPOP_E_INTERNAL with no partial results, like impop_pairwise_scan.
 * out_windows: one impop_kin_window per window; its sums run over all N(N-1)/2 pairs.  With m = min(het_i, het_j), a pair is
 * UNDEFINED in a window when m = 0 and RELATED when m > 0 and
 *     kin_den * (2 (het_het - 2 ibs0) + 2 m - het_i - het_j) >= 4 m kin_num          (int64, exact)
 * i.e. KING-robust kinship >= kin_num / kin_den (1 <= kin_den <= 2^20, 0 <= kin_num <= kin_den; else IMPOP_E_INVALID).
 * out_pairs (nullable): N(N-1)/2 records in the pair order of impop_scan_multi — (0,1),(0,2),..,(1,2),.. — each the nine cells
 * t[0][0], t[0][1], .., t[2][2] SUMMED OVER THE CALL'S WINDOWS; overlapping windows count as often as they occur.  One thread owns
 * an entry across a chunk's windows and adds integers: identical bytes from call to call.
 * out_watch (nullable with watch): n_windows x n_watch records, for the n_watch <= IMPOP_KINSHIP_MAX_WATCH listed pairs (i, j) of
 * individuals, in any order of i and j (het_i belongs to the first): local relatedness along the chromosome.  i == j, an index >=
 * N or n_watch above the limit return IMPOP_E_INVALID.
 * n_windows == 0 returns IMPOP_OK; windows may overlap and may be empty (every cell 0).  Chunking (IMPOP_PAIRWISE_CHUNK), uint16 or
 * int32 Gram counts, the Gram chain length, compaction of the source and the order of h1, h2 inside a pair never change a byte.
 * With impop_ctx_gram_timing on, impop_ctx_kinship_elapsed returns kernel_ms[0] = the plane builds, [1] = the epilogue kernels,
 * chunks = chunks timed, next to the Gram time.  Under IMPOP_TRACE=1 one line per call on stderr:
 *   [impop_kinship_scan] route=<dense|compact> individuals= rows= windows= chunks= launches= watch= plane_bytes=
 * Known answer (the rows of impop_diploid_scan's): h0 = 100010, h1 = 000010, h2 = 110000, h3 = 100001, pairs (0,1), (2,3), one
 * window [0, 6): genotypes g_0 = 1,0,0,0,2,0 and g_1 = 2,1,0,0,0,1, so t00 = 2, t01 = 2, t12 = 1, t20 = 1, the rest 0; het =
 * (1, 2), het_het = 0, ibs0 = 1, ibs2 = 2; KING within-family (het_het - 2 ibs0) / (het_i + het_j) = -2/3, KING-robust = -5/4. */
typedef struct impop_genotypes impop_genotypes;
int impop_genotypes_create(impop_ctx *ctx, const impop_matrix *m, const uint32_t *pairs /* h1,h2 per individual */, uint32_t n_ind,
                           impop_genotypes **out);
int impop_genotypes_info(const impop_genotypes *g, uint32_t *n_ind, uint64_t *n_site, uint64_t *device_bytes);
int impop_genotypes_download(impop_ctx *ctx, const impop_genotypes *g, uint64_t site_begin, uint64_t site_end,
                             uint64_t *bits_row_major /* 2N rows: H then A */, uint64_t row_stride_words);
int impop_genotypes_free(impop_ctx *ctx, impop_genotypes *g);
typedef struct impop_kinship_params {
    uint32_t struct_size;
    uint32_t kin_num, kin_den;          /* related: KING-robust kinship >= kin_num / kin_den */
    uint32_t reserved;
} impop_kinship_params;
typedef struct impop_kin_window {       /* 48 bytes, fixed layout: one per window */
    uint32_t n_ind;                     /* N */
    uint32_t n_sites;                   /* the window's W */
    uint64_t n_pairs;                   /* N (N - 1) / 2 */
    uint64_t het_het, ibs0, ibs2;       /* sums over all pairs */
    uint32_t n_related, n_undefined;    /* pairs at or above the threshold | with min(het_i, het_j) = 0 */
} impop_kin_window;
typedef struct impop_kin_pair {         /* 72 bytes, fixed layout: one per pair, summed over the call's windows */
    uint64_t t[9];                      /* t[3 a + b] */
} impop_kin_pair;
typedef struct impop_kin_watch {        /* 16 bytes, fixed layout: one per (window, watched pair) */
    uint32_t het_het, ibs0, het_i, het_j;
} impop_kin_watch;
int impop_kinship_scan(impop_ctx *ctx, const impop_genotypes *g, const impop_window *windows, uint64_t n_windows,
                       const impop_kinship_params *params, const uint32_t *watch /* 2 x n_watch individuals, nullable */,
                       uint32_t n_watch, impop_kin_window *out_windows, impop_kin_pair *out_pairs /* nullable */,
                       impop_kin_watch *out_watch /* nullable */);
#define IMPOP_HAPLOTYPE_MAX_N 4096u
/* Haplotype-frequency statistics per window from the stream impop_scan reads (no hap-major operand, no Gram; works on matrices
 * uploaded without IMPOP_KEEP_HAP_MAJOR, on compacted and on weighted ones).  Two members of P are the same haplotype in a window
 * iff their bits agree at every column of the window; site weights play no part in that, n_sites is the window's W as every other
 * record reports it (sum of weights, or the length).  Classes are ordered by (-size, smallest member index); class_of and sizes
 * have the layout and order of impop_cluster_scan's cluster_of and sizes, and at threshold 1.0 on the `match` identity that call
 * returns the same integers.  largest and second are the two largest sizes (second = 0 when there is one class).  The doubles
 * follow from the integers, with n = n_members, in this operation order:
 *     h1 = (double)sum_sq / ((double)n * (double)n)              h12 = h1 + 2.0 * ((double)largest / n) * ((double)second / n)
 *     h2_h1 = (h1 - ((double)largest / n) * ((double)largest / n)) / h1      hap_diversity = n < 2 ? 0.0 : (1.0 - h1) * n / (n - 1)
 * The result is exact: members are grouped by a 128-bit fingerprint of their bits, every group is then compared bit by bit with
 * its representative, and a window in which that comparison fails is regrouped by comparison alone.  A window without sites has
 * one class.  |P| = 0 returns IMPOP_E_INVALID, |P| > IMPOP_HAPLOTYPE_MAX_N IMPOP_E_UNSUPPORTED before anything is uploaded or
 * launched; n_windows == 0 returns IMPOP_OK.  Windows may overlap.  max_chunk_bytes (0 = 1 GiB) bounds the device memory of one
 * chunk of windows; chunking, the route (index, rows only, dense) and compaction never change a record. */
typedef struct impop_haplotype_params {
    uint32_t struct_size;
    uint32_t reserved;
    uint64_t max_chunk_bytes; /* 0 = default */
} impop_haplotype_params;
typedef struct impop_haplotype_stats { /* 64 bytes, fixed layout */
    uint32_t n_members, n_distinct, largest, second, n_singletons, n_sites;
    uint64_t sum_sq;          /* sum of size_k^2 */
    double h1, h12, h2_h1, hap_diversity;
} impop_haplotype_stats;
int impop_haplotype_scan(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows,
                         const uint64_t *mask_p, const impop_haplotype_params *params, impop_haplotype_stats *out_host,
                         uint32_t *class_of /* nullable, n_windows x |P| */, uint32_t *sizes /* nullable, n_windows x |P| */);
/* With impop_ctx_gram_timing on, impop_haplotype_scan brackets its kernels per chunk: kernel_ms[0] = fingerprints, [1] = grouping,
 * [2] = bitwise verification (and regrouping of flagged windows), summed since enable / reset; chunks = chunks timed. */
int impop_ctx_haplotype_elapsed(impop_ctx *ctx, double kernel_ms[3], uint64_t *chunks);
#define IMPOP_LD_MAX_N     4096u
#define IMPOP_LD_MAX_SITES 1024u
/* Linkage disequilibrium per window: Kelly's ZnS, mean |D'| and the Kim-Nielsen omega, from the site-major rows alone (no hap-major
 * operand, no Gram; works on full, weighted and compacted matrices).  Site weights play no part, a site is a column; n_sites is the
 * window's W as every other record reports it.
 * Site selection, per window: a site qualifies iff min(c, |P| - c) >= min_mac, c = its carriers among P.  The qualifying sites
 * are taken in ascending position and ranked 0..q-1; with m = min(q, max_sites) the site of rank floor(k q / m) (64-bit
 * integers; the identity when q <= max_sites) is used, k = 0..m-1.  n_qualifying = q, n_used = m.  used_sites (nullable,
 * n_windows x max_sites with max_sites as resolved, 0 -> 512) receives the ORIGINAL coordinates of the used sites: the first m
 * entries of a window's row are valid, the rest 0.
 * Pair arithmetic, used sites indexed 0..m-1 in position order, n = |P|, for sites s and t: c_s, c_t = carriers among P,
 * n11 = popcount(row_s & row_t & P),
 *     num = n n11 - c_s c_t (int64)             den = c_s (n - c_s) c_t (n - c_t) (int64)
 *     r2 = (double)(num num) / (double)den      (both below 2^53 for n <= 4096: one IEEE division of exact values)
 *     dmax = num > 0 ? min(c_s (n - c_t), (n - c_s) c_t) : min(c_s c_t, (n - c_s)(n - c_t))
 *     |D'| = (double)|num| / (double)dmax, 0.0 when num = 0
 * n_perfect counts the pairs with num num == den, n_complete those with num != 0 && |num| == dmax.  Either statistic is unchanged
 * when a site's alleles are flipped: stored polarity is irrelevant.
 * Sums, in this fixed order.  For site j: a_j = sum_{i<j} r2(i,j), i ascending from 0.0; b_j = sum_{k>j} r2(j,k), k ascending;
 * dp_j = sum_{i<j} |D'|(i,j), i ascending.  L(l) = sum_{j<l} a_j, j ascending; R(l) = sum_{j>=l} b_j, accumulated from j = m-1
 * downwards.  sum_r2 = L(m); sum_dprime = sum_j dp_j, j ascending; zns = sum_r2 / (m (m-1) / 2) and mean_dprime the same way,
 * both 0.0 when m < 2.
 * omega: for 2 <= l <= m-2, cross = (sum_r2 - L(l)) - R(l); a split with cross <= 0 is skipped, otherwise
 *     omega(l) = ((L(l) + R(l)) / (double)(C(l,2) + C(m-l,2))) / (cross / (double)(l (m-l)))
 * omega_max is the largest omega(l), omega_split its l (ties: the smallest l); both 0 when no split is defined.
 * Every pair is evaluated twice (once by each of its sites), so that a record needs no atomics and does not depend on scheduling.
 * |P| = 0, min_mac = 0, max_sites outside 4..IMPOP_LD_MAX_SITES (0 = 512) or a window outside the matrix return IMPOP_E_INVALID,
 * |P| > IMPOP_LD_MAX_N IMPOP_E_UNSUPPORTED, all before anything is uploaded or launched; n_windows == 0 returns IMPOP_OK.
 * Windows may overlap.  max_chunk_bytes (0 = 1 GiB) bounds the device memory of one chunk of windows; chunking, the upload's
 * keep flags and compaction never change a record (dropped sites are monomorphic and never qualify).  Checks the device error
 * word like impop_haplotype_scan (set when a window's gathered rows are not its n_used).
 * Under IMPOP_TRACE=1 the call prints one line on stderr:
 *   [impop_ld_scan] route=<dense|compact> windows= chunks= launches= qualifying= used= bytes_streamed= */
typedef struct impop_ld_params {
    uint32_t struct_size;
    uint32_t min_mac;         /* >= 1 */
    uint32_t max_sites;       /* 0 = 512; 4 .. IMPOP_LD_MAX_SITES */
    uint32_t reserved;
    uint64_t max_chunk_bytes; /* 0 = 1 GiB */
} impop_ld_params;
typedef struct impop_ld_stats { /* 72 bytes, fixed layout */
    uint32_t n_members, n_sites, n_qualifying, n_used, n_perfect, n_complete, omega_split, reserved;
    double sum_r2, sum_dprime, zns, mean_dprime, omega_max;
} impop_ld_stats;
int impop_ld_scan(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows, const uint64_t *mask_p,
                  const impop_ld_params *params, impop_ld_stats *out_host, uint64_t *used_sites /* nullable, n_windows x max_sites */);
/* With impop_ctx_gram_timing on, impop_ld_scan brackets its kernels per chunk: kernel_ms[0] = select, [1] = gather, [2] = pairs,
 * summed since enable / reset; chunks = chunks timed. */
int impop_ctx_ld_elapsed(impop_ctx *ctx, double kernel_ms[3], uint64_t *chunks);
#define IMPOP_RECOMB_MAX_N     4096u
#define IMPOP_RECOMB_MAX_SITES 16384u
/* Recombination per window under the infinite-sites model: the four-gamete test over all site pairs, Hudson & Kaplan's (1985)
 * lower bound R_min with its breakpoint intervals, four-gamete haplotype blocks (Wang et al. 2002) and Wall's (1999) B and Q, from
 * the site-major rows alone (works on full, weighted and compacted matrices; site weights change n_sites only).  Every device
 * output is an integer; the three doubles are one host operation each on those integers.
 * Members: P (mask_p; NULL = all), n = |P|.  Site selection is impop_ld_scan's rule: a site qualifies iff min(c, n - c) >= min_mac;
 * the qualifying sites are ranked by position 0..q-1 and with m = min(q, max_sites) the site of rank floor(k q / m) is used,
 * k = 0..m-1.  max_sites 0 means 4096; 2 .. IMPOP_RECOMB_MAX_SITES.  n_qualifying = q, n_used = m.  Thinning drops sites, never
 * adds an incompatible pair, so the R_min of a thinned window is still a valid lower bound on its recombination events.
 * Pair relations, used sites indexed 0..m-1 in position order, rows masked by P, for sites s and t:
 *     n11 = popcount(row_s & row_t)   n10 = c_s - n11   n01 = c_t - n11   n00 = n - c_s - c_t + n11
 *     incompatible(s,t) iff all four are > 0
 *     congruent(s,t)    iff (n10 == 0 && n01 == 0) || (n11 == 0 && n00 == 0): the same bipartition of P, so stored polarity is
 *                       irrelevant
 * Per site j (site_table, nullable, n_windows x max_sites):
 *     left1_j = 1 + max{ i < j : incompatible(i,j) }, 0 if there is none       n_left_j = #{ i < j : incompatible(i,j) }
 *     rep_j = min{ i <= j : congruent(i,j) }                                   carriers = c_j
 * Per window:
 *     n_incompatible = sum_j n_left_j        n_incompatible_adjacent = #{ j >= 1 : left1_j == j }
 *     rmin: cut = 0, r = 0; for j ascending: if left1_j >= 1 && left1_j - 1 >= cut then ++r, cut = j.  The chosen open intervals
 *       are (left1_j - 1, j); intervals that share an end point are disjoint, as in Hudson & Kaplan 1985.  The greedy equals the
 *       paper's deletion procedure and the maximum number of disjoint intervals among all incompatible pairs.
 *     blocks (pairwise compatible runs): M_j = max_{k<=j} left1_k; the longest compatible run ending at j is M_j..j.
 *       n_blocks = #{ j : j == m-1 or M_{j+1} > M_j } (the maximal runs); longest_block_sites = max_j (j - M_j + 1), ties to the
 *       smallest j; longest_block_begin / _end = the ORIGINAL coordinates of its first and last site.  All 0 when m = 0.
 *     Wall 1999: n_congruent_adjacent (B') = #{ j >= 1 : rep_j == rep_{j-1} }; n_partitions = #{ j : rep_j == j };
 *       n_congruent_partitions (A) = the distinct rep values among the sites of at least one congruent adjacent pair.
 *     four_gamete_fraction = n_incompatible / (m (m-1) / 2)   wall_b = B' / (m - 1)   wall_q = (B' + A) / m, each one IEEE
 *       division of exact values on the host, NaN where the denominator is 0.
 * Known answer: haplotypes h0..h3, five sites as rows over (h0,h1,h2,h3) 1100, 1010, 1100, 0011, 1000, min_mac 1, one window:
 *     left1 0,1,2,2,0   n_left 0,1,1,1,0   rep 0,1,0,0,4   n_incompatible 3   n_incompatible_adjacent 2   rmin 2 with the
 *     intervals (0,1) and (1,2)   n_blocks 3   longest block sites 2..4 (3)   B' 1   A 1   n_partitions 3   wall_b 0.25   wall_q 0.4
 * used_sites (nullable, n_windows x max_sites with max_sites as resolved) receives the ORIGINAL coordinates of the used sites;
 * entries of used_sites and site_table beyond n_used are 0.
 * |P| = 0, min_mac = 0, max_sites outside 2..IMPOP_RECOMB_MAX_SITES or a window outside the matrix return IMPOP_E_INVALID,
 * |P| > IMPOP_RECOMB_MAX_N IMPOP_E_UNSUPPORTED, all before anything is uploaded or launched; n_windows == 0 returns IMPOP_OK.
 * Windows may overlap.  max_chunk_bytes (0 = 1 GiB) bounds the device memory of one chunk of windows; chunking, the upload's keep
 * flags and compaction never change a record.  Checks the device error word like impop_ld_scan (set when a window's gathered rows
 * are not its n_used, or when rmin exceeds the number of sites with left1 > 0).
 * Under IMPOP_TRACE=1 the call prints one line on stderr:
 *   [impop_recomb_scan] route=<dense|compact> windows= chunks= launches= qualifying= used= pair_tiles= bytes_streamed=
 * pair_tiles = sum over the windows of ceil(n_used / 256), the tiles of sites the pair kernel worked on. */
typedef struct impop_recomb_params {
    uint32_t struct_size;
    uint32_t min_mac;         /* >= 1 */
    uint32_t max_sites;       /* 0 = 4096; 2 .. IMPOP_RECOMB_MAX_SITES */
    uint32_t reserved;
    uint64_t max_chunk_bytes; /* 0 = 1 GiB */
} impop_recomb_params;
typedef struct impop_recomb_stats { /* 96 bytes, fixed layout */
    uint32_t n_members, n_sites, n_qualifying, n_used, rmin, n_incompatible_adjacent, n_blocks, longest_block_sites,
        n_congruent_adjacent, n_congruent_partitions, n_partitions, reserved;
    uint64_t n_incompatible, longest_block_begin, longest_block_end;
    double four_gamete_fraction, wall_b, wall_q;
} impop_recomb_stats;
typedef struct impop_recomb_site { /* 16 bytes */
    uint32_t left1, n_left, rep, carriers;
} impop_recomb_site;
int impop_recomb_scan(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows, const uint64_t *mask_p,
                      const impop_recomb_params *params, impop_recomb_stats *out_host,
                      uint64_t *used_sites /* nullable, n_windows x max_sites */,
                      impop_recomb_site *site_table /* nullable, n_windows x max_sites */);
/* With impop_ctx_gram_timing on, impop_recomb_scan brackets its kernels per chunk: kernel_ms[0] = select, [1] = gather, [2] = pairs,
 * [3] = finish, summed since enable / reset; chunks = chunks timed. */
int impop_ctx_recomb_elapsed(impop_ctx *ctx, double kernel_ms[4], uint64_t *chunks);
#define IMPOP_LDBAND_MAX_N     4096u
#define IMPOP_LDBAND_MAX_BAND  1024u
#define IMPOP_LDBAND_MAX_BINS  4096u
#define IMPOP_LDBAND_FX_ONE    1073741824u   /* 2^30 */
/* Banded LD per window: r2 between every qualifying site and its next band_sites qualifying neighbours, with NO thinning, and from
 * that one object the LD decay curve (mean r2 by distance bin), per-site LD scores (Bulik-Sullivan et al. 2015) and a greedy LD
 * pruning of the sites.  Works on full, weighted and compacted matrices; site weights change n_sites only.  r2 is turned into a
 * fixed-point integer, so every device output is an integer and a plain restatement agrees bit for bit.
 * Members: P (mask_p; NULL = all), n = |P|.  A site of a window qualifies iff min(c, n - c) >= min_mac (impop_ld_scan's rule).
 * All q qualifying sites of the window are used, indexed 0..q-1 in position order; coord_j is the ORIGINAL coordinate of site j.
 * Band: the pair (j, k), j < k, is in the band iff k - j <= band_sites and (max_dist == 0 or coord_k - coord_j <= max_dist).
 * Pairs never cross windows; windows may overlap and are independent.
 * Pair arithmetic, rows masked by P: n11 = popcount(row_j & row_k)
 *     num = n n11 - c_j c_k      den = c_j (n - c_j) c_k (n - c_k)                     (impop_ld_scan's, in int64)
 *     r2 = (double)(num num) / (double)den      fx = (uint64_t)(r2 * 1073741824.0)     (0 <= fx <= IMPOP_LDBAND_FX_ONE)
 *     perfect iff num num == den       strong iff num num thr_den > thr_num den        (uint64; both products < 2^60)
 * Every quantity is invariant under flipping a site's alleles.
 * Decay bin of a pair: d = coord_k - coord_j, bin = min(d / bin_width, n_bins - 1) by integer division.
 * Pruning, greedy in position order (a fixed tie rule: the earlier site stays; no parity with PLINK's --indep-pairwise, which
 * removes by allele frequency inside sliding windows, is claimed): kept_0 = 1; kept_j = 1 iff there is no i < j with (i, j) in the
 * band, strong(i, j) and kept_i.  As a sliding window: K is a band_sites-bit register whose bit o-1 holds kept_{j-o}, strongmask_j
 * has bit o-1 set iff (j-o, j) is in the band and strong; kept_j = ((strongmask_j & K) == 0), then K = (K << 1) | kept_j.
 * Outputs: out_host[w] (n_pairs, sum_r2_fx, n_strong, n_perfect over the band pairs of the window; n_kept; site_off = the window's
 * first row in the site table = the sum of n_qualifying of the windows before it; mean_r2 = (double)sum_r2_fx / ((double)n_pairs *
 * 1073741824.0) on the host, NaN when n_pairs == 0).  bins (nullable, n_windows x n_bins): pairs, sum_r2_fx, n_strong of the band
 * pairs per decay bin.  site_table (nullable): one row per qualifying site of every window, windows in order, sites in position
 * order; ld_score_fx = the sum of fx over the site's band partners on BOTH sides, n_partners and n_strong count them likewise.
 * Capacity: *n_site_rows (nullable) always receives the sum of q; with site_table NULL or site_capacity below that sum nothing is
 * written to the table, the records and bins are filled all the same.
 * IMPOP_E_INVALID before anything is launched: a wrong struct_size, |P| = 0, min_mac = 0, band_sites outside
 * 1..IMPOP_LDBAND_MAX_BAND, n_bins outside 1..IMPOP_LDBAND_MAX_BINS, bin_width = 0, thr_den = 0, thr_den > 65535, thr_num > thr_den,
 * a window outside the matrix.  IMPOP_E_UNSUPPORTED before anything is launched: |P| > IMPOP_LDBAND_MAX_N.  n_windows == 0 returns
 * IMPOP_OK.  One refusal can only come AFTER the select pass, because q is not known before it: a single window whose q rows,
 * strong masks and site rows, q (4 ceil(n_hap / 32) + 8 ceil(band_sites / 64) + 32) bytes, exceed max_chunk_bytes (0 = 1 GiB),
 * or whose q band_sites >= 2^34, returns IMPOP_E_UNSUPPORTED with the numbers in the message.  The call counts q for every window
 * first and refuses before the first record, bin or table row is written: nothing is partially written.
 * Chunking, the LDS or global form of the decay counters (IMPOP_LDBAND_LDS_BINS=n lowers the bins the LDS form takes: a test aid),
 * the upload's keep flags and compaction never change a byte.  Checks the device error word (set when the rows gathered for a
 * window are not its q, when a window keeps more sites than it has, or when the site rows do not add up to twice the record).
 * Known answer: haplotypes h0..h3, five sites as rows over (h0,h1,h2,h3) 1100, 1010, 1100, 0011, 1000, one window, min_mac 1,
 * band_sites 4, max_dist 0, bin_width 2, n_bins 3, threshold 1/2.  r2: (0,2), (0,3), (2,3) give 1; (0,4), (1,4), (2,4), (3,4) give
 * 4/12, fx 357913941; the other three 0.  n_pairs 10, sum_r2_fx 4652881236, n_perfect 3, n_strong 3; kept 1,1,0,0,1, n_kept 3;
 * ld_score_fx 2505397589, 357913941, 2505397589, 2505397589, 1431655764; n_partners 4 each; bins (pairs, fx, strong)
 * (4, 1431655765, 1), (5, 2863311530, 2), (1, 357913941, 0).
 * Under IMPOP_TRACE=1 the call prints one line on stderr:
 *   [impop_ldband_scan] route=<dense|compact> windows= chunks= launches= qualifying= pairs= band= bins=<lds|global|off> bytes_streamed=
 * pairs = the sum of n_pairs; bins=off when bins is NULL; bytes_streamed = what the counting pass, the select and the gather
 * kernels read of the matrix plus the gathered rows. */
typedef struct impop_ldband_params {
    uint32_t struct_size;
    uint32_t min_mac;         /* >= 1 */
    uint32_t band_sites;      /* 1 .. IMPOP_LDBAND_MAX_BAND */
    uint32_t n_bins;          /* 1 .. IMPOP_LDBAND_MAX_BINS */
    uint32_t thr_num;         /* strong iff r2 > thr_num / thr_den; thr_num <= thr_den */
    uint32_t thr_den;         /* 1 .. 65535 */
    uint64_t bin_width;       /* >= 1, in coordinate units */
    uint64_t max_dist;        /* 0 = no distance limit */
    uint64_t max_chunk_bytes; /* 0 = 1 GiB */
} impop_ldband_params;
typedef struct impop_ldband_stats { /* 64 bytes, fixed layout */
    uint32_t n_members, n_sites, n_qualifying, n_kept;
    uint64_t n_pairs, sum_r2_fx, n_strong, n_perfect, site_off;
    double mean_r2;
} impop_ldband_stats;
typedef struct impop_ldband_bin { /* 24 bytes */
    uint64_t pairs, sum_r2_fx, n_strong;
} impop_ldband_bin;
typedef struct impop_ldband_site { /* 32 bytes */
    uint64_t coord, ld_score_fx;
    uint32_t carriers, n_partners, n_strong, kept;
} impop_ldband_site;
int impop_ldband_scan(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows, const uint64_t *mask_p,
                      const impop_ldband_params *params, impop_ldband_stats *out_host,
                      impop_ldband_bin *bins /* nullable, n_windows x n_bins */,
                      impop_ldband_site *site_table /* nullable, site_capacity rows */, uint64_t site_capacity,
                      uint64_t *n_site_rows /* nullable */);
/* With impop_ctx_gram_timing on, impop_ldband_scan brackets its kernels per chunk: kernel_ms[0] = select (the counting pass
 * included), [1] = rank + gather, [2] = pairs, [3] = prune, [4] = reduce, summed since enable / reset; chunks = chunks timed. */
int impop_ctx_ldband_elapsed(impop_ctx *ctx, double kernel_ms[5], uint64_t *chunks);
#define IMPOP_DIPLOID_MAX_N 2048u
/* The individual level of a windowed scan: observed heterozygosity, Wright's F_IS and runs of homozygosity per window and per
 * diploid individual, from the site-major rows alone (no hap-major operand, no Gram; works on full, weighted and compacted
 * matrices).  pairs lists 2 n_ind haplotype indices, (h1, h2) per individual; P = the 2N haplotypes of the pairs.  Haplotypes in
 * no pair play no part.  Site weights play no part either, a site is a column; n_sites is the window's W as every other record
 * reports it (sum of weights, or the length).
 * Per individual i of window [b, e): het = sites where bit(h1) != bit(h2), hom_alt = sites where both carry the allele.
 * Runs: let i be heterozygous at sites p_1 < ... < p_k of the window, in ORIGINAL site coordinates.  Its runs are p_1 - b, then
 * p_{j+1} - p_j - 1 for each j, then e - 1 - p_k; with k = 0 there is one run of length e - b.  Runs of length 0 are not runs.
 * longest_run = the longest run, roh_runs = the runs of at least min_run sites, roh_sites = the sites inside those.  On a
 * compacted matrix the coordinates are the kept sites' original positions, so the dropped monomorphic sites lie inside runs, as
 * they should.
 * Per window: s_p and sum_p are impop_window_stats' for P = the pairs (c_s = carriers among the 2N), het_sites = sites at which at
 * least one individual is heterozygous, the other integers sum (longest_run: maximise) the individuals' rows.  The doubles are
 * computed on the host from the integers, with L = seq_len if it is greater than 0, else W, and n = 2N, in exactly this order:
 *     ho    = (double)het_total / ((double)N * L)
 *     he    = 2.0 * (double)sum_p / ((double)n * (n - 1) * L)
 *     f_is  = 1.0 - (double)(het_total * (n - 1)) / (double)sum_p          NaN when sum_p == 0
 *     f_roh = (double)roh_sites_total / ((double)N * W)                    NaN when W == 0
 * All device output is integers: a plain host restatement of the definitions agrees bit for bit.
 * Known answer: haplotype rows over 6 sites h0 = 100010, h1 = 000010, h2 = 110000, h3 = 100001 (site 0 first), pairs (0,1) and
 * (2,3), one window [0, 6), min_run = 3, seq_len = 0.  Individual 0: het 1, hom_alt 1, longest_run 5, roh_runs 1, roh_sites 5;
 * individual 1: het 2, hom_alt 1, longest_run 3, roh_runs 1, roh_sites 3.  Window: s_p 4, het_sites 3, het_total 3, sum_p 13,
 * roh_sites_total 8, roh_runs_total 2, longest_run 5, ho 0.25, he 26/72, f_is 1 - 9/13, f_roh 8/12.
 * n_ind == 0, min_run == 0, a wrong struct_size, an index >= n_hap, h1 == h2, a haplotype in two pairs or a window outside the
 * matrix return IMPOP_E_INVALID, n_ind > IMPOP_DIPLOID_MAX_N IMPOP_E_UNSUPPORTED, all before anything is uploaded or launched;
 * n_windows == 0 returns IMPOP_OK.  Windows may overlap and may hold one site.  max_chunk_bytes (0 = 1 GiB) bounds the device
 * memory of one chunk of windows; chunking, the upload's keep flags and compaction never change a record.  Checks the device
 * error word like impop_haplotype_scan (set when a window's het_total is not the sum of its rows' het, or a row's run lengths
 * and het do not add up to the window's length).
 * ind_out (nullable): n_windows x n_ind rows, individual-minor, in the order of `pairs`.
 * Under IMPOP_TRACE=1 the call prints one line on stderr:
 *   [impop_diploid_scan] route=<dense|compact> windows= tiles= chunks= launches= individuals= bytes_streamed= */
typedef struct impop_diploid_params {
    uint32_t struct_size;
    uint32_t min_run;          /* >= 1: a homozygous run counts as ROH when it is at least this many sites long */
    uint64_t max_chunk_bytes;  /* 0 = 1 GiB */
} impop_diploid_params;
typedef struct impop_diploid_stats {   /* 80 bytes, fixed layout, one per window */
    uint32_t n_ind, n_sites;           /* N, W */
    uint32_t s_p;                      /* sites with 0 < c < 2N among the 2N haplotypes of the pairs */
    uint32_t het_sites;                /* sites at which at least one individual is heterozygous */
    uint64_t het_total;                /* sum over individuals of het_i */
    uint64_t sum_p;                    /* sum_s c_s (2N - c_s): same quantity as impop_window_stats.sum_p for P = the pairs */
    uint64_t roh_sites_total;          /* sum over individuals of roh_sites_i */
    uint32_t roh_runs_total;           /* sum over individuals of roh_runs_i */
    uint32_t longest_run;              /* max over individuals of longest_run_i */
    double ho, he, f_is, f_roh;        /* host, from the integers, see above */
} impop_diploid_stats;
typedef struct impop_diploid_ind {     /* 24 bytes, optional table, n_windows x N, individual-minor */
    uint32_t het;          /* sites where bit(h1) != bit(h2) */
    uint32_t hom_alt;      /* sites where both carry the allele */
    uint32_t longest_run;  /* longest stretch of window sites with no heterozygous site */
    uint32_t roh_runs;     /* number of such stretches >= min_run */
    uint32_t roh_sites;    /* sites inside them */
    uint32_t reserved;     /* 0 */
} impop_diploid_ind;
int impop_diploid_scan(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows,
                       const uint32_t *pairs /* 2N haplotype indices: h1,h2 per individual */, uint32_t n_ind,
                       const impop_diploid_params *params, impop_diploid_stats *out, impop_diploid_ind *ind_out /* nullable */);
/* With impop_ctx_gram_timing on, impop_diploid_scan brackets its kernels per chunk: kernel_ms[0] = tile summaries, [1] = window
 * records, summed since enable / reset; chunks = chunks timed. */
int impop_ctx_diploid_elapsed(impop_ctx *ctx, double kernel_ms[2], uint64_t *chunks);
#define IMPOP_IBS_MAX_N     4096u        /* |P| in the all-pairs form */
#define IMPOP_IBS_MAX_PAIRS 8388608u     /* pairs per call, either form (>= C(4096,2)) */
#define IMPOP_IBS_OPEN_LEFT  1u          /* tract begins at site_begin: cut by the range, not by a difference */
#define IMPOP_IBS_OPEN_RIGHT 2u          /* tract ends at site_end */
/* Pairwise identity-by-state tracts over a whole range of sites in one pass: where two haplotypes are identical, and for how
 * long.  Between the two copies of one sample these are the runs of homozygosity as segments.  Works on full, weighted and
 * compacted matrices, from the site-major rows alone (no hap-major operand).
 * Pairs: either every pair i < j of the members of mask_p (NULL = all haplotypes), i-major in ascending haplotype order, or,
 * with pairs non-NULL, the n_pairs listed (h1, h2); n_pairs is ignored in the all-pairs form.  A pair may repeat and a
 * haplotype may be in any number of pairs.  Swapping h1 and h2 changes nothing but the two fields.
 * Definition: for pair (h1, h2) and range [b, e) = [site_begin, site_end) let p_1 < ... < p_k be the sites of the range where
 * the two rows differ.  The tracts are [b, p_1), (p_j + 1 .. p_{j+1}) for each j and [p_k + 1, e); with k = 0 there is one tract
 * [b, e).  Tracts of length 0 are not tracts.  These are impop_diploid_scan's runs for the "individual" (h1, h2) and window
 * [b, e).  Reported tracts are those with end - begin >= min_sites; n_diff and longest do not depend on min_sites.  The segment
 * list is pair-major, ascending begin inside a pair.  Site weights play no part (n_sites of a window record is its W as every
 * other record reports it).  On a compacted matrix the coordinates are the kept sites' original positions, so dropped
 * monomorphic sites lie inside tracts.  site_end - site_begin must be below 2^32.
 * Segment capacity: *n_segments always receives the total.  When seg_out is NULL or seg_capacity is smaller than the total, the
 * call returns IMPOP_OK and writes nothing to seg_out; pair_out and win_out are filled all the same, so the caller can call
 * again with room.  The device never writes a segment past what the counting sweep announced: a mismatch between the two sweeps
 * sets the device error word and the call returns IMPOP_E_INTERNAL.
 * Window records are integer sums over the REPORTED tracts, formed with integer atomics and sums only, whether or not the
 * segment list is returned; no per-site array over the range is used, and chunking never changes them.  An empty window gets
 * zeros and share = NaN.
 * Known answer: rows over 6 sites, site 0 first, h0 = 100010, h1 = 000010, h2 = 110000, h3 = 100001; all pairs, range [0, 6),
 * min_sites = 2.  (0,1): n_diff 1, longest 5, tract [1,6) OPEN_RIGHT; (0,2): 2, 2, [2,4); (0,3): 2, 4, [0,4) OPEN_LEFT;
 * (1,2): 3, 2, [2,4); (1,3): 3, 3, [1,4); (2,3): 2, 3, [2,5).  Six segments, 19 tract sites.  Windows (pair_sites, tracts,
 * pairs_spanning): [0,6) -> (19, 6, 0); [2,4) -> (12, 6, 6); [3,6) -> (9, 6, 1).
 * A wrong struct_size, min_sites == 0, an empty or out-of-matrix range, h1 == h2, an index >= n_hap, both pairs and mask_p,
 * fewer than 2 members (or n_pairs == 0), a window not inside the range and a win_out / windows nullness mismatch return
 * IMPOP_E_INVALID; |P| > IMPOP_IBS_MAX_N and n_pairs > IMPOP_IBS_MAX_PAIRS IMPOP_E_UNSUPPORTED; all before anything is uploaded
 * or launched.  max_chunk_bytes (0 = 1 GiB) bounds the transposed words of one chunk of sites plus the segment staging of one
 * range of pairs.  IMPOP_IBS_CHUNK_BLOCKS=n (1..4096) sets the site-chunk length in 64-site blocks and IMPOP_IBS_SEG_BLOCKS=n
 * the length of the sub-segments of a chunk that run in parallel (test aids); records never change with either.
 * Under IMPOP_TRACE=1 the call prints one line on stderr:
 *   [impop_ibs_scan] route=<dense|compact> pairs= site_chunks= sub_segments= launches= tracts= bytes_streamed=
 * (bytes_streamed: the site-major rows the transposes read plus the transposed words the walks read). */
typedef struct impop_ibs_params {        /* 32 bytes */
    uint32_t struct_size;
    uint32_t min_sites;                  /* >= 1: a tract is reported when it is at least this many sites long */
    uint64_t site_begin, site_end;       /* the range, ORIGINAL site coordinates; site_end == 0: the matrix's end */
    uint64_t max_chunk_bytes;            /* 0 = 1 GiB: bounds the device memory of one chunk */
} impop_ibs_params;
typedef struct impop_ibs_pair {          /* 32 bytes, fixed layout, one per pair, in pair order */
    uint32_t h1, h2;
    uint32_t n_diff;                     /* sites of the range where the two rows differ */
    uint32_t longest;                    /* longest tract of any length (0 when the rows differ at every site) */
    uint32_t n_tracts;                   /* tracts >= min_sites */
    uint32_t reserved;
    uint64_t tract_sites;                /* sites inside those */
} impop_ibs_pair;
typedef struct impop_ibs_segment {       /* 32 bytes, fixed layout */
    uint32_t h1, h2;
    uint64_t begin, end;                 /* [begin, end), ORIGINAL coordinates */
    uint32_t pair;                       /* index into the pair order */
    uint32_t flags;                      /* IMPOP_IBS_OPEN_* */
} impop_ibs_segment;
typedef struct impop_ibs_window {        /* 32 bytes, fixed layout, one per window */
    uint64_t pair_sites;                 /* sum over reported tracts of |tract intersected with the window| */
    uint32_t tracts;                     /* reported tracts that meet the window */
    uint32_t pairs_spanning;             /* reported tracts that contain the whole window (at most one per pair) */
    uint32_t n_sites, reserved;          /* W as every other record reports it */
    double share;                        /* host: (double)pair_sites / ((double)n_pairs * (double)(end - begin)); NaN for an empty window */
} impop_ibs_window;
int impop_ibs_scan(impop_ctx *ctx, const impop_matrix *m,
                   const uint64_t *mask_p,            /* all-pairs form: pairs i < j of the members, i-major; NULL = all haplotypes */
                   const uint32_t *pairs, uint64_t n_pairs,   /* list form: h1,h2 per pair; non-NULL excludes mask_p */
                   const impop_window *windows, uint64_t n_windows,   /* nullable */
                   const impop_ibs_params *params,
                   impop_ibs_pair *pair_out,          /* nullable */
                   impop_ibs_segment *seg_out, uint64_t seg_capacity, uint64_t *n_segments,
                   impop_ibs_window *win_out);        /* n_windows records; NULL iff windows is NULL */
/* With impop_ctx_gram_timing on, impop_ibs_scan brackets its kernels: kernel_ms[0] = transposes, [1] = the walks of both sweeps,
 * [2] = combine / close kernels, summed since enable / reset; chunks = site chunks transposed (both sweeps counted). */
int impop_ctx_ibs_elapsed(impop_ctx *ctx, double kernel_ms[3], uint64_t *chunks);
#define IMPOP_IBD_MAX_MAP 4194304u       /* breakpoints of a genetic map (2^22) */
/* Identity-by-descent segments of pairs of haplotypes: impop_ibs_scan's exact tracts joined across short gaps, with lengths
 * measured on a genetic map.  The rule is the seed-and-extend rule of hap-IBD (Zhou, Browning & Browning 2020) written as a pure
 * function of a pair's exact tracts; it is integer-exact.  No parity with that program's output is claimed: this definition is
 * the contract.  Matrix, range [b, e) = [site_begin, site_end), pairs (member mask or list) and windows are impop_ibs_scan's.
 * Map (optional): n_map breakpoints (pos_k, g_k), pos strictly ascending in ORIGINAL site coordinates, g non-decreasing uint64 in
 * the caller's length unit (the command line uses micro-centimorgans).  G(x) = g_0 for x <= pos_0, g_last for x >= pos_last, else
 * with pos_k <= x < pos_{k+1}: G(x) = g_k + floor((x - pos_k) (g_{k+1} - g_k) / (pos_{k+1} - pos_k)) in uint64.  A map with a pos
 * or g step >= 2^32 is refused (the product cannot overflow), as are n_map == 1 and n_map > IMPOP_IBD_MAX_MAP.  Without a map
 * (both pointers NULL, n_map 0) G(x) = x.
 * Tracts of a pair: exactly impop_ibs_scan's tracts of [b, e) before any length filter.  The LENGTH of [s, t) is G(t) - G(s), its
 * EXTENT t - s.
 * Candidate: a tract with extent >= min_sites (>= 1) and length >= min_extend.  Seed: a candidate with length >= min_seed;
 * min_seed < min_extend is refused.
 * Chain: a maximal run of consecutive candidates of the pair in which each next candidate begins at most max_gap coordinates
 * after the previous one ends (gap = next.begin - prev.end >= 1, so max_gap = 0 never joins).  Non-candidate tracts and
 * discordant sites between two candidates lie inside the gap.
 * IBD segment: a chain that holds at least one seed and has G(end) - G(begin) >= min_output, begin = the first candidate's
 * begin, end = the last candidate's end; len = G(end) - G(begin), n_tracts = its candidates, ibs_sites = the sum of their
 * extents, flags = IMPOP_IBS_OPEN_LEFT / _RIGHT when begin == b / end == e.  Site weights play no part; on a compacted matrix
 * the coordinates are the kept sites' original positions.  The list is pair-major, ascending inside a pair.
 * Known answers: two rows over 40 sites, h0 all 0, h1 with 1 at sites 10, 12 and 30; pair (0,1), range [0,40): the tracts are
 * [0,10), [11,12), [13,30), [31,40).
 *   (a) no map, min_sites 2, min_extend 5, min_seed 12, min_output 20: max_gap 3 gives one segment [0,40), len 40, n_tracts 3,
 *       ibs_sites 36, open on both sides; max_gap 2 gives one segment [13,40), len 27, n_tracts 2, ibs_sites 26, OPEN_RIGHT (the
 *       chain {[0,10)} has no seed); max_gap 2 with min_output 30 gives nothing.
 *   (b) map (0,0),(20,100),(40,120), so G(13) = 65, G(30) = 110, G(31) = 111; min_sites 2, min_extend 10, min_seed 40,
 *       min_output 50, max_gap 3: [31,40) has length 9 and is no candidate; one segment [0,30), len 110, n_tracts 2,
 *       ibs_sites 27, OPEN_LEFT.
 * Cost: the tracts of extent >= min_sites are staged on the device (impop_ibs_scan's two sweeps, a range of pairs at a time) and
 * one wave per pair chains them; min_sites is the cost lever: with min_sites = 1 every tract is staged.
 * Capacity: as impop_ibs_scan.  *n_segments always receives the total; seg_out is written only when seg_capacity >= total;
 * pair_out and win_out are filled either way.  Window records are impop_ibs_window with "reported tract" read as "IBD segment".
 * Everything impop_ibs_scan refuses, a bad map and min_seed < min_extend return IMPOP_E_INVALID; |P| > IMPOP_IBS_MAX_N, n_pairs >
 * IMPOP_IBS_MAX_PAIRS and n_map > IMPOP_IBD_MAX_MAP IMPOP_E_UNSUPPORTED; all before anything is uploaded or launched.  A segment
 * the counting pass did not announce is never written: the device error word is set and the call returns IMPOP_E_INTERNAL.
 * Under IMPOP_TRACE=1 the call prints one line on stderr:
 *   [impop_ibd_scan] route=<dense|compact> pairs= pair_ranges= candidates= segments= map_points= launches= bytes_streamed=
 * (candidates: the tracts that passed extent and min_extend; map_points: the breakpoints uploaded, those that bracket the range). */
typedef struct impop_ibd_params {        /* 88 bytes */
    uint32_t struct_size;
    uint32_t min_sites;                  /* >= 1: extent a candidate needs; the tracts staged */
    uint64_t site_begin, site_end;       /* as impop_ibs_params */
    uint64_t min_seed, min_extend, min_output;   /* units of G */
    uint64_t max_gap;                    /* coordinates */
    const uint64_t *map_pos, *map_g;     /* n_map each, or both NULL */
    uint32_t n_map, reserved;
    uint64_t max_chunk_bytes;            /* as impop_ibs_params */
} impop_ibd_params;
typedef struct impop_ibd_pair {          /* 48 bytes, fixed layout, one per pair, in pair order */
    uint32_t h1, h2;
    uint32_t n_segments;                 /* IBD segments of the pair */
    uint32_t n_candidates;               /* its candidate tracts, in a reported chain or not */
    uint64_t total_len, total_extent, longest_len, ibs_sites;   /* over the reported segments: sums of len, end - begin, the largest len, sum of ibs_sites */
} impop_ibd_pair;
typedef struct impop_ibd_segment {       /* 48 bytes, fixed layout */
    uint32_t h1, h2;
    uint64_t begin, end;                 /* [begin, end), ORIGINAL coordinates */
    uint64_t len;                        /* G(end) - G(begin) */
    uint32_t ibs_sites, n_tracts;        /* over the chain's candidates */
    uint32_t pair;                       /* index into the pair order */
    uint32_t flags;                      /* IMPOP_IBS_OPEN_* */
} impop_ibd_segment;
int impop_ibd_scan(impop_ctx *ctx, const impop_matrix *m,
                   const uint64_t *mask_p, const uint32_t *pairs, uint64_t n_pairs,   /* as impop_ibs_scan */
                   const impop_window *windows, uint64_t n_windows,   /* nullable */
                   const impop_ibd_params *params,
                   impop_ibd_pair *pair_out,          /* nullable */
                   impop_ibd_segment *seg_out, uint64_t seg_capacity, uint64_t *n_segments,
                   impop_ibs_window *win_out);        /* n_windows records; NULL iff windows is NULL */
/* With impop_ctx_gram_timing on: kernel_ms[0] = transposes, [1] = walks, [2] = combine / close, [3] = the chain kernel (both
 * forms), summed since enable / reset; chunks = site chunks transposed. */
int impop_ctx_ibd_elapsed(impop_ctx *ctx, double kernel_ms[4], uint64_t *chunks);
#define IMPOP_PAINT_MAX_DONORS     1024u     /* admissible donors per recipient */
#define IMPOP_PAINT_MAX_RECIPIENTS 4096u
#define IMPOP_PAINT_MAX_PANELS     8u
#define IMPOP_PAINT_MAX_COST       1048576u  /* 2^20: the largest switch cost */
#define IMPOP_PAINT_NO_PANEL       255u
/* Chromosome painting: every recipient haplotype as a mosaic of donor haplotypes, the Li & Stephens (2003) copying model read as
 * a Viterbi path with integer costs (a min-plus recursion).  Every output is an integer; ties fall by the rules below.
 * Inputs: the matrix m and the range [b, e) = [site_begin, site_end) as impop_ibs_scan; a donor mask mask_d over the haplotypes
 * (NULL = all); n_rec recipient haplotypes, which may also be donors; optionally group[h] (uint32 per haplotype, NULL means
 * group[h] = h) and panel[h] (uint8 per haplotype, 0 .. n_panels - 1, IMPOP_PAINT_NO_PANEL = no panel; n_panels <= 8).
 * Admissible donors: donor j is admissible for recipient i iff j is in mask_d and group[j] != group[i].  So a haplotype never
 * copies from itself, and with sample groups never from the other haplotype of its own individual.  Admissible donors are ordered
 * by haplotype index.  Each recipient needs at least 1.
 * Sites and coordinates: the sites s = 0 .. L-1 are the stored sites of the range; on a compacted matrix they are the kept sites
 * and coord(s) is their original coordinate, as in impop_ibs_scan.  Site weights play no part.
 * Costs: mu = mismatch_cost, 1 <= mu <= 65535.  c_s, the cost of changing donor between site s-1 and s (s >= 1), is the constant
 * switch_cost or, with site_switch_cost non-NULL, site_switch_cost[s]: one uint32 per stored site of the range (n_site_switch_cost
 * must be L), entry 0 ignored.  Every c_s lies in 0 .. IMPOP_PAINT_MAX_COST.
 * Recursion, for recipient i over its admissible donors j:
 *     V_j(0) = mu * [x_i(0) != x_j(0)]
 *     M(s)   = min_j V_j(s)            A(s) = the LOWEST admissible j with V_j(s) = M(s)
 *     stay_j(s) = ( V_j(s-1) <= M(s-1) + c_s )                    (a tie stays)
 *     V_j(s) = mu * [x_i(s) != x_j(s)] + min( V_j(s-1), M(s-1) + c_s )
 *     path:  d(L-1) = A(L-1);   d(s-1) = d(s) if stay_{d(s)}(s) else A(s-1)
 *     cost = M(L-1)   (uint64)
 * Segments: a segment is a maximal run [s0, s1) of constant d; adjacent segments always differ in donor.  begin = coord(s0), or b
 * for the first segment; end = coord(s1), or e for the last, so a recipient's segments tile [b, e); n_sites = s1 - s0; n_mismatch
 * = the sites of the run where recipient and donor differ.  The segment list is recipient-major, ascending.
 * Segment capacity: as impop_ibs_scan.  *n_segments always receives the total; seg_out is written only when seg_capacity >= the
 * total; every other output is filled either way.
 * chunk_counts[n_rec][n_hap] (uint32) = the segments recipient r copies from haplotype h; chunk_sites[n_rec][n_hap] (uint64) = the
 * sites of those segments (ChromoPainter's chunk-count and chunk-length matrices, with lengths in sites).
 * Windows [wb, we), original coordinates, any list (overlapping, irregular, empty, outside the range): a site belongs to a window
 * iff its coordinate lies in it.  A window record sums over all recipients: n_switches = the sites s >= 1 with d(s) != d(s-1),
 * n_mismatch, cells = recipients x sites, copied[p] = the cells whose donor has panel p (slot 8: no panel).
 * anc[n_windows][n_rec][n_panels + 1] (uint32) = the same split per recipient, slot n_panels = no panel: the local-ancestry table.
 * Known answers: h0 = 000000000100, h1 = 000000111111, h2 = 111111000000, h3 = 111111111011 (site 0 first), recipient h0, donors
 * {1, 2, 3}, dense, range [0, 12).  mu 1, c 2: cost 3, n_mismatch 1, segments h1 [0,6), h2 [6,12).  mu 3, c 1: cost 3, n_mismatch
 * 0, h1 [0,6), h2 [6,9), h1 [9,10), h2 [10,12).  mu 1, c 5: cost 5, n_mismatch 5, h1 [0,12).  With every donor identical to the
 * recipient: one segment from the lowest admissible donor, cost 0.
 * What it is not: it is not the posterior (forward-backward) painting; it has no stay-probability term beyond what the caller
 * folds into c_s; no parity with ChromoPainter's output is claimed: this definition is the contract.
 * IMPOP_E_INVALID: a wrong struct_size, an empty or out-of-matrix range (or one of 2^32 sites or more, or, on a compacted matrix,
 * one without a kept site), n_rec == 0, a recipient index out of range or repeated, a recipient without an admissible donor, mu
 * or a switch cost outside its range, n_site_switch_cost != L, n_panels > 0 without panel or a panel value that is neither
 * < n_panels nor 255, windows / win_out / anc_out nullness that does not go together.  IMPOP_E_UNSUPPORTED: more than
 * IMPOP_PAINT_MAX_DONORS admissible donors of a recipient, n_rec > IMPOP_PAINT_MAX_RECIPIENTS, n_panels > IMPOP_PAINT_MAX_PANELS.
 * All before anything is uploaded or launched.
 * Cost: O(recipients x donors x sites), serial along the sites.  One wave holds a recipient's states in registers; per site it
 * writes 8 bytes (A(s) and the site where that state's segment began), from which the path falls out in one jump per segment.
 * Recipients run in ranges whose per-site records fit half of max_chunk_bytes (0 = 1 GiB), the sites in chunks of 64-site blocks
 * whose transposed words fit the other half; IMPOP_PAINT_CHUNK_BLOCKS=n (1..4096) sets the chunk length (test aid).  Records never
 * change with either.  The emit pass recomputes mu * n_mismatch + the switch costs of every path from the words; where that is not
 * the forward pass's cost, a recipient's n_sites do not sum to L or a segment was not announced by the count, the device error
 * word is set, nothing unannounced is written and the call returns IMPOP_E_INTERNAL.
 * Under IMPOP_TRACE=1 the call prints one line on stderr:
 *   [impop_paint_scan] route=<dense|compact> recipients= donors= sites= site_chunks= recipient_ranges= segments= launches= bytes_streamed=
 * (donors: the members of mask_d; site_chunks: chunks transposed, all passes; bytes_streamed: rows read by the transposes plus
 * words read by the forward kernel). */
typedef struct impop_paint_params {      /* 72 bytes */
    uint32_t struct_size;
    uint32_t mismatch_cost;              /* mu, 1 .. 65535 */
    uint32_t switch_cost;                /* c, 0 .. IMPOP_PAINT_MAX_COST; ignored when site_switch_cost is given */
    uint32_t n_panels;                   /* 0 .. IMPOP_PAINT_MAX_PANELS */
    uint64_t site_begin, site_end;       /* the range, ORIGINAL site coordinates; site_end == 0: the matrix's end */
    const uint32_t *site_switch_cost;    /* nullable: c_s per stored site of the range */
    uint64_t n_site_switch_cost;         /* its stated length: must be L */
    const uint32_t *group;               /* nullable: n_hap entries */
    const uint8_t *panel;                /* nullable: n_hap entries */
    uint64_t max_chunk_bytes;            /* 0 = 1 GiB */
} impop_paint_params;
typedef struct impop_paint_recipient {   /* 40 bytes, fixed layout, one per recipient, in the caller's order */
    uint32_t h;
    uint32_t n_donors;                   /* admissible donors */
    uint32_t n_segments;
    uint32_t n_mismatch;
    uint32_t distinct_donors;
    uint32_t longest_sites;              /* the longest segment's n_sites (the first of equals) */
    uint32_t longest_donor;              /* and its donor */
    uint32_t reserved;
    uint64_t cost;                       /* M(L-1) */
} impop_paint_recipient;
typedef struct impop_paint_segment {     /* 40 bytes, fixed layout */
    uint32_t h, donor;                   /* recipient and donor haplotype */
    uint64_t begin, end;                 /* [begin, end), ORIGINAL coordinates */
    uint32_t n_sites, n_mismatch;
    uint32_t recipient;                  /* index into the recipient list */
    uint32_t reserved;
} impop_paint_segment;
typedef struct impop_paint_window {      /* 96 bytes, fixed layout, one per window */
    uint64_t n_switches, n_mismatch, cells;
    uint64_t copied[9];                  /* cells by the donor's panel; slot 8 = no panel */
} impop_paint_window;
int impop_paint_scan(impop_ctx *ctx, const impop_matrix *m,
                     const uint64_t *mask_d,                       /* donors; NULL = all haplotypes */
                     const uint32_t *recipients, uint32_t n_rec,
                     const impop_window *windows, uint64_t n_windows,   /* nullable */
                     const impop_paint_params *params,
                     impop_paint_recipient *rec_out,               /* nullable */
                     impop_paint_segment *seg_out, uint64_t seg_capacity, uint64_t *n_segments,
                     uint32_t *chunk_counts, uint64_t *chunk_sites,   /* nullable, n_rec x n_hap each */
                     impop_paint_window *win_out,                  /* nullable; needs windows */
                     uint32_t *anc_out);                           /* nullable; needs windows */
/* With impop_ctx_gram_timing on: kernel_ms[0] = transposes, [1] = the forward kernel, [2] = backtrack (count + emit), mismatch and
 * record kernels, [3] = the window kernel, summed since enable / reset; chunks = site chunks the forward kernel ran. */
int impop_ctx_paint_elapsed(impop_ctx *ctx, double kernel_ms[4], uint64_t *chunks);
#define IMPOP_DSTAT_GROUP 3u   /* quartets whose sums one streaming launch of impop_dstat_scan keeps in registers */
#define IMPOP_DSTAT_MAX_QUARTETS 64u
/* Introgression statistics per window and quartet of populations (P1, P2, P3, O): Patterson's D (ABBA-BABA), f4 and Martin's f_d,
 * from one streaming pass over the scan's own stream (the variable-site index with its rare entries where the matrix has one:
 * every term is zero at a site that is monomorphic among all haplotypes, so that route is exact; weighted matrices stream the
 * rows, compacted ones their kept sites).  masks holds n_pop (4..8) bitsets of ceil(n_hap / 64) words, quartets n_quartets
 * (1..IMPOP_DSTAT_MAX_QUARTETS) x {P1, P2, P3, O} indices into masks.  The four populations of a quartet are pairwise disjoint;
 * populations that never share a quartet may overlap.  A quartet may be listed twice.
 * Per site s and quartet, c_k = carriers of allele 1 among population k (n_k members), w_s = the site's weight (1 without
 * weights).  polarize = 1 takes the outgroup's major allele as ancestral, per site and quartet: 2 cO > nO turns every c_k into
 * n_k - c_k, 2 cO == nO leaves the site out of that quartet's sums and counts it in n_skipped.  Then
 *     abba      = sum_s w_s (n1 - c1) c2 c3 (nO - cO)            baba = sum_s w_s c1 (n2 - c2) c3 (nO - cO)
 *     f4_num    = sum_s w_s (c1 n2 - c2 n1) (c3 nO - cO n3)
 *     fd_den_p2 = sum over the sites with c2 n3 >= c3 n2 of w_s (c2 n1 - c1 n2) c2 (nO - cO)
 *     fd_den_p3 = sum over the other sites              of w_s (c3 n1 - c1 n3) c3 (nO - cO)
 * (fd_den_*: Martin's S(P1, P_D, P_D, O) with the donor P_D the one of P2 / P3 with the higher frequency, a tie to P2), and
 * n_informative = the sites (columns, not weights) whose abba + baba term is positive.  Every integer is exact: neither the
 * route, the tiling nor the order of summation enters a record.  The doubles are computed on the host from the integers, in
 * exactly this order:
 *     d  = (double)(abba - baba) / (double)(abba + baba)                                   NaN when abba + baba == 0
 *     f4 = (double)f4_num / (double)(n1 n2 n3 nO)
 *     fd = ((double)(abba - baba) / (double)(n1 n2 n3 nO)) /
 *          ((double)fd_den_p2 / (double)(n1 n2 n2 nO) + (double)fd_den_p3 / (double)(n1 n3 n3 nO))    NaN when that sum is 0
 * Known answer: eight haplotypes, P1 = {0,1}, P2 = {2,3}, P3 = {4,5}, O = {6,7}; six sites with the counts (c1, c2, c3, cO) =
 * (0,2,2,0) (2,0,2,0) (1,2,1,0) (0,1,2,0) (1,1,0,0) (2,2,2,2), the carriers of a population its lowest-numbered haplotypes; one
 * window [0, 6).  Quartet (P1,P2,P3,O): abba 28, baba 16, f4_num -12, fd_den_p2 24, fd_den_p3 16, n_informative 4, n_skipped 0,
 * d = 12/44 = 3/11, f4 = -0.75, fd = 0.3.  Quartet (P2,P1,P3,O): abba 16, baba 28, f4_num 12, fd_den_p2 12, fd_den_p3 8,
 * d = -3/11, fd = -0.6.  polarize = 1 gives the same records (the last site turns into all zeros, no outgroup count is a tie).
 * n_pop outside 4..8, n_quartets outside 1..IMPOP_DSTAT_MAX_QUARTETS, a wrong struct_size, an empty population, a quartet index
 * >= n_pop, a quartet whose populations are not pairwise disjoint, a window outside the matrix and n_hap > 65535 return
 * IMPOP_E_INVALID; IMPOP_E_UNSUPPORTED when n1 nO max(n2, n3)^2 times the largest window's weight sum is not below 2^62 (the
 * message names the quartet and the window: no sum can wrap); all before anything is uploaded or launched.  n_windows == 0
 * returns IMPOP_OK.  Windows may overlap and may hold one site.
 * The quartets are handled IMPOP_DSTAT_GROUP at a time: one streaming launch and one finalize launch per group, on the same
 * tiles.  tile_blocks (0 = default; the environment's IMPOP_DSTAT_TILE_BLOCKS=1..4096 overrides it) bounds a tile's 64-site
 * blocks.  Checks the device error word like impop_haplotype_scan.  out_host: n_windows x n_quartets records, window-major.
 * Under IMPOP_TRACE=1 the call prints one line on stderr:
 *   [impop_dstat_scan] route=<indexed+rare|indexed|dense|compact> windows= tiles= quartets= launches= bytes_streamed= */
typedef struct impop_dstat_params {
    uint32_t struct_size;
    int32_t  polarize;     /* 0: allele 1 is the derived allele as stored; 1: the outgroup's major allele is ancestral */
    uint32_t tile_blocks;  /* 0 = default */
    uint32_t reserved;
} impop_dstat_params;
typedef struct impop_dstat_stats {   /* 80 bytes, fixed layout */
    uint32_t n_sites;        /* as impop_window_stats.n_sites */
    uint32_t n_informative;  /* sites (not weights) with abba + baba term > 0 */
    uint32_t n_skipped;      /* polarize ties */
    uint32_t flags;          /* 0 */
    int64_t  abba;           /* sum_s w_s (n1-c1) c2 c3 (nO-cO) */
    int64_t  baba;           /* sum_s w_s c1 (n2-c2) c3 (nO-cO) */
    int64_t  f4_num;         /* sum_s w_s (c1 n2 - c2 n1)(c3 nO - cO n3) */
    int64_t  fd_den_p2;      /* sites with c2 n3 >= c3 n2: sum w_s (c2 n1 - c1 n2) c2 (nO-cO) */
    int64_t  fd_den_p3;      /* the other sites:           sum w_s (c3 n1 - c1 n3) c3 (nO-cO) */
    double   d, f4, fd;      /* host, from the integers, see above */
} impop_dstat_stats;
int impop_dstat_scan(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows,
                     const uint64_t *masks, uint32_t n_pop, const uint32_t *quartets /* n_quartets x {P1,P2,P3,O} */,
                     uint32_t n_quartets, const impop_dstat_params *params, impop_dstat_stats *out_host /* [window][quartet] */);
/* With impop_ctx_gram_timing on, impop_dstat_scan brackets its streaming launches: their summed time and number since enable /
 * reset. */
int impop_ctx_dstat_elapsed(impop_ctx *ctx, double *total_ms, uint64_t *launches);
#define IMPOP_SFS_PAIR_GROUP 4u   /* pairs whose counters one streaming launch of impop_sfs_scan keeps in registers */
#define IMPOP_SFS_MAX_PAIRS 28u
#define IMPOP_SFS_TABLE_1D 1u     /* impop_sfs_params.tables: bit 0 the 1-D spectra, bit 1 the joint spectra */
#define IMPOP_SFS_TABLE_JOINT 2u
/* Everything read from the site-frequency spectrum, per window: every population's spectrum summaries and neutrality statistics
 * (Watterson's theta, theta_pi, theta_H, theta_L, Tajima's D, Fay & Wu's H, its normalised form and Zeng's E), every requested
 * pair's Wakeley-Hey site classes, and optionally the 1-D and the joint spectra as tables; from the scan's own stream like
 * impop_dstat_scan (indexed+rare, indexed, dense, compact, weighted).  masks holds n_pop (1..8) bitsets of ceil(n_hap / 64)
 * words, every population non-empty; pairs holds n_pairs (0..IMPOP_SFS_MAX_PAIRS) x {a, b} indices into masks, a != b, the two
 * populations of a pair disjoint (populations that share no pair may overlap); outgroup = a population index, or -1 for none.
 * Per site, c_k = carriers of allele 1 among population k (n_k members).  With an outgroup O: 2 c_O == n_O makes the site a TIE,
 * which adds 1 to n_skipped and to nothing else; 2 c_O > n_O turns every c_k into n_k - c_k (the outgroup's major allele is
 * ancestral).  Without an outgroup the counts are taken as stored: the folded quantities (seg, sum_het, theta_w, theta_pi,
 * tajima_d, the pair classes) do not depend on polarity, while eta1, eta_n1, sum_c, sum_c2, theta_h, theta_l, faywu_h,
 * faywu_h_norm and zeng_e are meaningful only if allele 1 is the derived allele.  A site that is monomorphic among all haplotypes
 * adds nothing to any field and is never a tie (its outgroup count is 0 or n_O), so the variable-site index and a compaction
 * are exact.
 * Per (window, population k), impop_sfs_stats: seg = #{0 < c_k < n_k}; over those segregating sites eta1 = #{c_k == 1},
 * eta_n1 = #{c_k == n_k - 1}, sum_het = sum c (n - c), sum_c = sum c, sum_c2 = sum c^2.  On a weighted matrix the three sums
 * carry the site weight, every counter and every table counts columns, n_sites is the window's weight sum.  The doubles are
 * computed on the host from the integers, in one place (csrc/sfs_math.h), in exactly this order, with S = seg, n = n_k:
 *     a1 = sum_{i=1}^{n-1} 1/i, a2 = sum 1/i^2 (ascending); b1, b2, c1, c2, e1, e2 as for impop_window_stats.tajima_d
 *     P = n (n - 1) / 2
 *     theta_w  = S / a1              theta_pi = sum_het / P         theta_h = sum_c2 / P         theta_l = sum_c / (n - 1)
 *     tajima_d = (theta_pi - theta_w) / sqrt(e1 S + e2 S (S - 1))
 *     T2 = S (S - 1) / (a1^2 + a2)   b = a2 + 1 / n^2
 *     faywu_h  = theta_pi - theta_h
 *     var_H = (n - 2) / (6 (n - 1)) theta_w + [18 n^2 (3 n + 2) b - (88 n^3 + 9 n^2 - 13 n + 6)] / (9 n (n - 1)^2) T2
 *     faywu_h_norm = (theta_pi - theta_l) / sqrt(var_H)
 *     var_E = (n / (2 (n - 1)) - 1 / a1) theta_w
 *             + [a2 / a1^2 + 2 (n / (n - 1))^2 a2 - 2 (n a2 - n + 1) / ((n - 1) a1) - (3 n + 1) / (n - 1)] T2
 *     zeng_e = (theta_l - theta_w) / sqrt(var_E)
 * (the variances: Zeng et al. 2006, eqs. 14 and 12).  n < 2: all eight doubles are NaN.  A ratio (tajima_d, faywu_h_norm,
 * zeng_e) is NaN when S == 0 or when its variance is <= 0 or not finite (n = 2 and n = 3 make some of them exactly 0).
 * Per (window, pair (A, B)), impop_sfs_pair: private_a = A segregates and B does not, private_b the mirror case, shared = both
 * segregate, fixed_a = c_A == n_A and c_B == 0, fixed_b = c_A == 0 and c_B == n_B, n_union = the sum of the five: exactly the
 * sites that segregate in A + B.
 * Tables (uint32, counting columns): sfs_out[w] concatenates the K spectra, n_k + 1 bins each; bin c counts the sites with
 * c_k == c and 0 < c < n_k, bins 0 and n_k are 0 (so a population's spectrum does not depend on the other populations of the
 * call).  jsfs_out[w] concatenates, per pair, an (n_A + 1) x (n_B + 1) table, row-major in c_A, over the pair's n_union sites:
 * [0][0] and [n_A][n_B] are 0.
 * Every integer is exact: neither the route, the tiling, the chunking nor the order of summation enters a record or a table.
 * Known answer: 12 haplotypes, A = {0..4}, B = {5..9}, O = {10,11}, the carriers of a population its lowest-numbered members; 11
 * sites with (c_A, c_B, c_O) = (1,0,0) (2,1,0) (5,0,0) (0,4,0) (1,1,1) (3,5,2) (0,0,0) (5,5,2) (0,0,1) (4,2,0) (0,5,2); one window
 * [0, 11), pair (A, B).  Without an outgroup (seg, eta1, eta_n1, sum_het, sum_c, sum_c2): A 5 2 1 24 11 31, B 4 2 1 18 8 22,
 * O 2 2 2 2 2 2; pair: private_a 2, private_b 1, shared 3, fixed_a 1, fixed_b 1, n_union 8; joint cells, one each: (0,4) (0,5)
 * (1,0) (1,1) (2,1) (3,5) (4,2) (5,0).  A: theta_pi 2.4, theta_h 3.1, theta_l 2.75, faywu_h -0.7.  B: theta_w 1.92, theta_pi 1.8,
 * tajima_d -0.41017465, faywu_h_norm -0.34892049, zeng_e 0.13767880.  With outgroup O, n_skipped is 2: A 4 1 1 20 9 25,
 * B 3 1 1 14 7 21, O 0 0 0 0 0 0; pair: private_a 2, private_b 1, shared 2, fixed_a 2, fixed_b 0, n_union 7; joint cells (0,4)
 * (1,0) (2,0) (2,1) (4,2) and (5,0) twice.  A: tajima_d 0.27344977, faywu_h -0.5, faywu_h_norm -0.43615061, zeng_e 0.56792505.
 * A wrong struct_size, n_pop outside 1..8, n_pairs above IMPOP_SFS_MAX_PAIRS, an empty population, a pair with a == b or an index
 * >= n_pop, a pair whose populations share a haplotype, outgroup >= n_pop (or below -1), n_hap > 65535, a window outside the
 * matrix, tables bit 1 with n_pairs == 0 and a requested table whose pointer is NULL return IMPOP_E_INVALID;
 * IMPOP_E_UNSUPPORTED unless n_k^2 times the largest window's weight sum is below 2^62 (the message names the population and
 * the window: no sum can wrap); all before anything is uploaded or launched.  n_windows == 0 returns IMPOP_OK.
 * The summary pass handles the pair list IMPOP_SFS_PAIR_GROUP at a time, all populations in the first launch: one streaming and
 * one finalize launch per group, on the same tiles.  The table pass runs one job per requested table (a population's spectrum,
 * a pair's joint spectrum) over (window, part) items, a part being a run of the window's tiles: a workgroup tallies its item
 * into a histogram in LDS and adds the non-zero bins to the window's table with integer atomics; a job whose bins do not fit the
 * LDS (the environment's IMPOP_SFS_LDS_BINS=0..40960 caps what the LDS form takes, a test aid) tallies straight into the table.
 * Tables come down per chunk of windows; max_chunk_bytes (0 = 1 GiB) bounds the device memory of a chunk's tables.  tile_blocks
 * (0 = default; the environment's IMPOP_SFS_TILE_BLOCKS=1..4096 overrides it) bounds a tile's 64-site blocks.  Checks the
 * device error word like impop_haplotype_scan.  Under IMPOP_TRACE=1 the call prints one line on stderr:
 *   [impop_sfs_scan] route=<indexed+rare|indexed|dense|compact> windows= tiles= pops= pairs= launches= table_jobs= lds_jobs=
 *                    table_items= chunks= bytes_streamed= table_bytes_streamed=
 * (table_bytes_streamed: what the table pass reads, overlapping windows re-reading the tiles they share). */
typedef struct impop_sfs_params {     /* 24 bytes */
    uint32_t struct_size;
    int32_t  outgroup;         /* population index whose major allele is ancestral, -1: none (counts as stored) */
    uint32_t tile_blocks;      /* 0 = default */
    uint32_t tables;           /* IMPOP_SFS_TABLE_* bits */
    uint64_t max_chunk_bytes;  /* 0 = 1 GiB */
} impop_sfs_params;
typedef struct impop_sfs_stats {      /* 112 bytes, fixed layout, [window][population] */
    uint32_t n_sites;          /* as impop_window_stats.n_sites */
    uint32_t seg;              /* sites with 0 < c < n */
    uint32_t eta1;             /* of those, c == 1 */
    uint32_t eta_n1;           /* of those, c == n - 1 */
    uint32_t n_skipped;        /* outgroup ties of the window */
    uint32_t flags;            /* 0 */
    uint64_t sum_het;          /* sum w_s c (n - c) over the segregating sites */
    uint64_t sum_c;            /* sum w_s c */
    uint64_t sum_c2;           /* sum w_s c^2 */
    double theta_w, theta_pi, theta_h, theta_l, tajima_d, faywu_h, faywu_h_norm, zeng_e;   /* host, from the integers, see above */
} impop_sfs_stats;
typedef struct impop_sfs_pair {       /* 32 bytes, fixed layout, [window][pair] */
    uint32_t private_a, private_b, shared, fixed_a, fixed_b, n_union;
    uint32_t n_skipped;        /* outgroup ties of the window */
    uint32_t flags;            /* 0 */
} impop_sfs_pair;
int impop_sfs_scan(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows, const uint64_t *masks,
                   uint32_t n_pop, const uint32_t *pairs /* 2 x n_pairs, nullable */, uint32_t n_pairs, const impop_sfs_params *params,
                   impop_sfs_stats *stats_out /* n_windows x n_pop */, impop_sfs_pair *pairs_out /* n_windows x n_pairs, nullable */,
                   uint32_t *sfs_out /* nullable */, uint32_t *jsfs_out /* nullable */);
/* The eight doubles of an impop_sfs_stats record from its integers (host only, no context), in the record's order: theta_w,
 * theta_pi, theta_h, theta_l, tajima_d, faywu_h, faywu_h_norm, zeng_e. */
int impop_sfs_neutrality(uint32_t n, uint64_t seg, uint64_t sum_het, uint64_t sum_c, uint64_t sum_c2, double out[8]);
/* With impop_ctx_gram_timing on, impop_sfs_scan brackets its streaming launches: kernel_ms[0] = the summary pass, [1] = the table
 * pass, summed since enable / reset; launches = the summary launches timed. */
int impop_ctx_sfs_elapsed(impop_ctx *ctx, double kernel_ms[2], uint64_t *launches);
/* Measurement aid (like impop_scan_plan_timing): with timing enabled every Gram launch of impop_pairwise_scan on this context
 * is bracketed with hipEvents on the context's stream; elapsed() synchronises and returns the summed Gram-kernel time and the
 * number of launches since enable / reset. */
/* Test aid: ORs `bits` into the context's device error word, as a kernel whose consistency check trips would; the next call
 * that checks the word (impop_pairwise_scan, impop_pi_from_identity, impop_fst_grouped_from_identity) returns
 * IMPOP_E_INTERNAL and clears it. */
int impop_debug_raise_device_error(impop_ctx *ctx, uint32_t bits);
int impop_ctx_gram_timing(impop_ctx *ctx, int enable);
int impop_ctx_gram_elapsed(impop_ctx *ctx, double *total_ms, uint64_t *launches);
/* With the same switch on, impop_cluster_scan also brackets its clustering kernel(s): their summed time and number of
 * chunks since enable / reset, next to the Gram time above. */
int impop_ctx_cluster_elapsed(impop_ctx *ctx, double *total_ms, uint64_t *launches);
/* ... and impop_pairdist_scan its distribution kernel: summed time and number of chunks since enable / reset. */
int impop_ctx_pairdist_elapsed(impop_ctx *ctx, double *total_ms, uint64_t *launches);
/* ... and impop_genotypes_create its plane-build kernel, impop_kinship_scan its epilogue kernels: kernel_ms[0] = plane builds,
 * [1] = epilogue, summed since enable / reset; chunks = chunks of impop_kinship_scan timed. */
int impop_ctx_kinship_elapsed(impop_ctx *ctx, double kernel_ms[2], uint64_t *chunks);
/* ... and impop_pca_scan its two kernels: kernel_ms[0] = the eigen kernel of every chunk, [1] = the distance kernel, summed since
 * enable / reset; chunks = eigen launches timed. */
int impop_ctx_pca_elapsed(impop_ctx *ctx, double kernel_ms[2] /* eigen kernel, distance kernel */, uint64_t *chunks);
/* ... and impop_tree_scan its tree kernel: summed time and number of chunks since enable / reset. */
int impop_ctx_tree_elapsed(impop_ctx *ctx, double *total_ms, uint64_t *launches);
/* ... and impop_permtest_scan its two kernels: kernel_ms[0] = the preparation kernel, [1] = the labelling kernel of every chunk,
 * summed since enable / reset; chunks = chunks timed. */
int impop_ctx_permtest_elapsed(impop_ctx *ctx, double kernel_ms[2] /* preparation, labelling */, uint64_t *chunks);
/* Test aid: how many event pairs the four timers hold (created on first timed use, kept for reuse): sizes[0..2] = the
 * context's Gram / clustering / EHH timers, sizes[3] = the plan's (plan nullable: 0).  Nothing is created while timing is off. */
int impop_debug_timer_pool_sizes(const impop_ctx *ctx, const impop_scan_plan *plan, uint64_t sizes[4]);

/* impop_pairwise_scan over several devices, sharded like impop_scan_sharded (declared with the multi-GPU entry points
 * above; run_pica2_impg.sh:125-236 / run_h-fst.sh:155-190 with thresholds):
 * shard k = the windows impop_shard_windows gives it, contracted on ctxs[k] from slabs[k] (which needs its hap-major
 * operand, IMPOP_KEEP_HAP_MAJOR).  Every shard runs on a host thread of its own, so the devices work side by side;
 * contexts must be distinct.  out_host: n_windows records in the order of `windows`, byte for byte what one context
 * holding the whole matrix returns. */
int impop_pairwise_scan_sharded(impop_ctx *const *ctxs, const impop_matrix *const *slabs, const uint64_t *slab_site_begin,
                                int n_ctx, const impop_window *windows, uint64_t n_windows, const uint64_t *mask_p,
                                const uint64_t *mask_a, const uint64_t *mask_b, const impop_pairwise_params *params,
                                impop_pairwise_stats *out_host);


/* ---- statistics on a given identity matrix (the .sim drop-in path) ---------
 * These take what read_similarity_file (pica2.py:6-58, h-fst.py:84-119) yields,
 * densified by the caller, and run the reference's arithmetic on the GPU. */

/* pica2.analyze_similarity_matrix (pica2.py:60-169).  seq_len 0 = None.
 * group_of (nullable, n entries): 0-based index of each element's group in the
 * reference's sorted group order (pica2.py:110-112).
 * seed_rank (nullable, n entries, distinct values): the order in which the greedy grouping of
 * pica2.py:96-110 takes its seeds.  The reference takes them with set.pop() from `remaining =
 * set(elements)`, which walks the set's hash table from slot 0 without ever rehashing, so its seed order is
 * the iteration order of `set(elements)` restricted to what is left; a caller in the same interpreter passes
 * seed_rank[i] = position of element i in list(set(elements)) and gets the reference's groups for
 * non-transitive tables too (impop_amd/pica2.py does).  NULL = seed with the smallest remaining index
 * (lexicographically smallest name): deterministic, and one of the orders the reference can take.
 * detail (nullable): the two intermediate values pica2's log prints (pica2.py:158-159). */
typedef struct impop_pica2_detail {
    double sum_2pairs;          /* sum(2 * pair for pair in group_pairs) */
    uint64_t n_pairs_with_data; /* len(group_pairs) */
} impop_pica2_detail;
int impop_pi_from_identity(impop_ctx *ctx, const double *ident, uint32_t n, double threshold, int round_digits,
                           uint64_t seq_len, const uint32_t *seed_rank, double *pi, double *pi_site, uint32_t *group_of,
                           uint32_t *n_groups, impop_pica2_detail *detail);
/* The "Step 2" table of pica2's log (pica2.py:125-145) for given groups: rep[g] = index of group g's first
 * member, group_size[g]; for the pairs g < h in row-major order sims_out = identity of the two
 * representatives (rounded like the analysis; NaN = pair absent) and values_out = (1 - sim) * f_g * f_h.
 * Both arrays hold n_groups*(n_groups-1)/2 doubles.  n_groups < 2: there is no pair, nothing is written and the call
 * returns IMPOP_OK.  A rep[g] >= n, or group sizes that sum to 0, return IMPOP_E_INVALID before anything is launched. */
int impop_pica2_pair_terms(impop_ctx *ctx, const double *ident, uint32_t n, int round_digits, const uint32_t *rep,
                           const uint32_t *group_size, uint32_t n_groups, double *sims_out, double *values_out);

/* h-fst.calculate_fst (h-fst.py:173-249).  in_a / in_b: n membership flags.
 * out[6] = fst, pi_a, pi_b, pi_xy, dxy, da.
 * counts[6] = pairs_a, missing_a, pairs_b, missing_b, pairs_between, missing_between. */
int impop_fst_from_identity(impop_ctx *ctx, const double *ident, uint32_t n, const uint8_t *in_a,
                            const uint8_t *in_b, uint64_t seq_len, int round_digits, double *out,
                            uint64_t *counts);

/* scripts/hudson/hud.py calculate_fst(method='grouped') (hud.py:64-128, 173-300): greedy groups
 * inside each population at `threshold`, frequency-weighted group-pair sums; the similarity of two
 * groups is the first pair (members in sorted order) present in the table.  out[6] as above;
 * counts[6] = groups_a, missing_a, groups_b, missing_b, group pairs between, missing between.
 * seed_rank (nullable, n entries): seed order of hud.py:64-86's set.pop() inside each population, as for
 * impop_pi_from_identity — values must be distinct among the members of A and among those of B (position
 * in list(set(pop_a)) / list(set(pop_b))); entries of non-members are ignored. */
int impop_fst_grouped_from_identity(impop_ctx *ctx, const double *ident, uint32_t n, const uint8_t *in_a,
                                    const uint8_t *in_b, double threshold, uint64_t seq_len, int round_digits,
                                    const uint32_t *seed_rank, double *out, uint64_t *counts);

/* tj_d.tajimas_d (tj_d.py:47-69) for `count` (n, S, pi) triples.  comps
 * (nullable): count x 10 doubles a1,a2,b1,b2,c1,c2,e1,e2,numerator,denominator.
 * Returns IMPOP_E_INVALID (message = the reference's ValueError text) if any
 * triple has n < 2, S < 0 or pi < 0; nothing is written in that case. */
int impop_tajimas_d(impop_ctx *ctx, const int64_t *n, const double *S, const double *pi, uint64_t count,
                    double *D, double *comps);

/* ---- a ragged batch of identity tables (one `.sim` table per window) ------------
 * pica2, h-fst and Tajima's D for k tables of different size, names and seed order in one call: per chunk of tables one
 * upload of the matrices, one of the side tables, two kernel launches whatever the number of tables, one download.
 * Chunks are capped by the bytes they upload (max_chunk_bytes; 0 = the size of the context's scratch, at least 128 MiB);
 * chunking never changes a record.  Staging goes through the context's page-locked buffer.
 * Per problem: pica2 as impop_pi_from_identity (threshold, round_digits, seq_len, seed_rank); with in_a / in_b also
 * h-fst as impop_fst_from_identity (fst_round_digits; the same seq_len) — without them fst[] is NaN and fst_counts[] 0;
 * with tajima_n >= 2 also Tajima's D as impop_tajimas_d(tajima_n, tajima_S, pi) with pi = pi_site through its "%.8f" text
 * (run_tajd.sh:174-180) — else, or for a negative S or a NaN pi_site, tajima_d is NaN.
 * Supported n per problem: 0 .. 1023.  A larger problem gets status = IMPOP_E_UNSUPPORTED in its own record (every other
 * field 0) and does not fail the call: send it through the single-problem entry points.
 * group_of (nullable): the problems' n group indices back to back, in problem order.
 * Checks the device error word like impop_pi_from_identity.
 * Under IMPOP_TRACE=1 every chunk prints one line on stderr:
 *   [impop_sim_batch] tables=<in the chunk> chunk=<index> bytes_up=<uploaded> launches=<kernel launches> max_n=<largest n>
 *                     stage_us=<host copy into the staging buffer> up_us= kernels_us= down_us=<GPU time of each phase> */
typedef struct impop_identity_problem {
    const double *ident;        /* n x n row-major, NaN = pair absent; NULL allowed when n == 0 */
    uint32_t n, reserved;
    uint64_t seq_len;           /* 0 = None */
    const uint32_t *seed_rank;  /* nullable; n distinct values, as impop_pi_from_identity */
    const uint8_t *in_a, *in_b; /* n flags each; both or neither */
    int64_t tajima_n;           /* < 2 = no D */
    double tajima_S;
} impop_identity_problem;
#define IMPOP_IDENTITY_STATS_BYTES 144
typedef struct impop_identity_stats { /* 144 bytes, fixed layout */
    int32_t status;             /* IMPOP_OK or IMPOP_E_UNSUPPORTED */
    uint32_t n_groups;
    double pi, pi_site, sum_2pairs;
    uint64_t n_pairs_with_data;
    double fst[6];              /* fst, pi_a, pi_b, pi_xy, dxy, da */
    uint64_t fst_counts[6];     /* pairs_a, missing_a, pairs_b, missing_b, pairs_between, missing_between */
    double tajima_d;
} impop_identity_stats;
typedef struct impop_identity_batch_params {
    uint32_t struct_size;       /* sizeof(impop_identity_batch_params) */
    int32_t round_digits;       /* pica2 rounding, < 0 = none */
    double threshold;
    int32_t fst_round_digits;   /* h-fst rounding, < 0 = none */
    uint32_t reserved;
    uint64_t max_chunk_bytes;   /* 0 = default */
} impop_identity_batch_params;
int impop_stats_from_identity_batch(impop_ctx *ctx, const impop_identity_problem *problems, uint64_t k,
                                    const impop_identity_batch_params *params, impop_identity_stats *out,
                                    uint32_t *group_of);
/* The tajima_d of a batch record as host arithmetic (no device needed): Tajima's D for (n, S) and pi = pi_site rounded
 * through its "%.8f" text; NaN for n < 2, S < 0, or a negative or NaN pi_site. */
int impop_tajimas_d_from_pi_site(int64_t n, double S, double pi_site, double *D);

/* af.cluster (af.py:35-44): connected components of {identity >= threshold}
 * ordered by (-size, members); cluster_of[i] = 0-based cluster rank (c1 = 0),
 * sizes (nullable): n entries, first n_clusters valid.
 * i and j are linked when EITHER ident[i*n+j] or ident[j*n+i] is a number >= threshold: a table that holds only
 * one orientation of a pair (NaN in the other) clusters like the symmetric one.
 * n <= IMPOP_CLUSTER_MAX_N (the labels of all samples stay in the LDS of one workgroup); a larger n returns
 * IMPOP_E_INVALID before anything is uploaded or launched. */
int impop_cluster_from_identity(impop_ctx *ctx, const double *ident, uint32_t n, double threshold,
                                uint32_t *cluster_of, uint32_t *n_clusters, uint32_t *sizes);

/* ---- native .sim ingest (host code) ------------------------------------------
 * Replaces pica2.read_similarity_file (pica2.py:6-58) / h-fst.read_similarity_file
 * (h-fst.py:84-119) for clean tab-separated files.  flavor 0 = pica2 (the first
 * unparsable value stops the parse: bad_line / impop_sim_bad_text report it, the
 * caller prints the reference's message and exits 1), flavor 1 = h-fst (unparsable
 * values are skipped and counted in n_bad).  Returns IMPOP_E_UNSUPPORTED for any file
 * shape it is not certain CPython's csv + float() would read identically (quotes,
 * short rows, unusual number syntax, missing columns): the caller then uses the
 * Python reader.  A missing file returns IMPOP_E_INVALID. */
typedef struct impop_sim impop_sim;
int impop_sim_parse(const char *path, int flavor, impop_sim **out);
int impop_sim_info(const impop_sim *s, uint32_t *n_names, uint64_t *n_rows, uint64_t *names_bytes,
                   int64_t *bad_line, uint64_t *n_bad);
int impop_sim_names(const impop_sim *s, char *buf);          /* NUL-separated, sorted */
/* first_seen_out[k] (n_names entries) = sorted rank of the k-th distinct name in file order (group.a before
 * group.b within a row): the insertion order of the reference reader's `elements` set (pica2.py:45-46),
 * from which the caller rebuilds that set and hence pica2's seed order (see impop_pi_from_identity). */
int impop_sim_first_seen(const impop_sim *s, uint32_t *first_seen_out);
int impop_sim_bad_text(const impop_sim *s, char *buf, size_t buflen);
int impop_sim_dense(const impop_sim *s, double *out);        /* n x n, sorted-name order, NaN = absent */
int impop_sim_free(impop_sim *s);
/* impop_sim_parse on k files with at most n_threads worker threads (0 = OMP_NUM_THREADS if set, else 16; never the
 * machine's core count).  out[i] / rc_out[i] are what impop_sim_parse(paths[i], flavor, ..) gives (out[i] NULL where
 * rc_out[i] != 0; IMPOP_E_NOMEM for a file whose parse ran out of memory).  Returns IMPOP_OK unless an argument is bad;
 * per-file failures are in rc_out. */
int impop_sim_parse_many(const char *const *paths, uint64_t k, int flavor, int n_threads, impop_sim **out, int *rc_out);

/* ---- native GFA ingest (host code) ---------------------------------------------
 * S / P / W lines of the window graph (`impg query -o gfa`, run_tajd.sh:126; `odgi view -g`, :140) -> the NODE-level
 * presence matrix: rows = paths and walks sorted by name (W named sample#hap#seqid[:start-end]), columns = segments
 * (decimal ids in numeric order, then the others), bit-packed hap-major as impop_matrix_upload takes it; the segment
 * lengths are the site weights of impop_matrix_set_site_weights.  ref_prefix (nullable): the first path whose name
 * starts with it gives every column a reference coordinate (start parsed from a trailing ":start-end"; columns off
 * the reference inherit the preceding one; non-decreasing).  Same rules as impop_amd/extract.py:from_gfa
 * (expand_bp=False), which the caller falls back to on ANY non-zero status (so error texts stay Python's). */
typedef struct impop_gfa impop_gfa;
int impop_gfa_parse(const char *path, const char *ref_prefix, impop_gfa **out);
int impop_gfa_info(const impop_gfa *g, uint32_t *n_path, uint64_t *n_seg, uint64_t *names_bytes, int64_t *ref_row);
int impop_gfa_names(const impop_gfa *g, char *buf);                       /* NUL-separated, row order */
int impop_gfa_bits(const impop_gfa *g, uint64_t *bits_hap_major, uint64_t row_stride_words);
int impop_gfa_lengths(const impop_gfa *g, uint32_t *lengths);            /* per column */
int impop_gfa_positions(const impop_gfa *g, int64_t *positions);         /* per column; needs ref_prefix */
int impop_gfa_free(impop_gfa *g);
/* `odgi paths -H` table (header row; path.name, path.length, node.count; then one 0 / visit-count column per node — the
 * shape scripts/wip/op-afs.py:112 reads) -> the same handle: rows sorted by name, one column per node (all lengths 1,
 * no positions).  Rows are parsed by several host threads.  Same rules as impop_amd/extract.py:from_paths_table, which
 * the caller falls back to on ANY non-zero status. */
int impop_paths_table_parse(const char *path, impop_gfa **out);

/* CPython round(x, ndigits) (pica2.py:83, h-fst.py:150) evaluated on the GPU,
 * exposed so that the device implementation can be fuzzed against CPython. */
int impop_py_round(impop_ctx *ctx, const double *x, uint64_t count, int ndigits, double *out);

#define IMPOP_IHS_SCAN_MAX_N 4096u       /* |P| */
#define IMPOP_IHS_EDGE_BITS  0x00FFu     /* flags: the integral ran into the end of the site range */
#define IMPOP_IHS_LIMIT_BITS 0xFF00u     /* flags: the integral ran into max_extend_* */
/* Per-site integrated haplotype homozygosity for a whole range of sites in one pass: the integers behind iHS and nSL (one
 * population, classes by allele) and XP-EHH / XP-nSL (two populations, classes by population), with the EHH cutoff.  The device
 * carries a positional Burrows-Wheeler transform over the sites that vary in P, so neighbouring cores share all their work and
 * every number is an exact integer.  Works on full, weighted and compacted matrices (site weights play no part).
 * Populations: mask_b NULL: K = 1, P = the members of mask_a (NULL = all haplotypes).  Else K = 2: A = mask_a, B = mask_b,
 * disjoint, at least 2 members each, P = A u B.
 * Stepped sites: the sites s of [site_begin, site_end) (site_end 0 = the matrix's end; ORIGINAL coordinates) with
 * 0 < c_P(s) < |P|, numbered 0, 1, ... in order (ordinals); p(x) = the coordinate of ordinal x.  Sites monomorphic in P are
 * never stepped on.  Cores: the stepped sites inside [core_begin, core_end) (core_end 0 = site_end) with
 * min(c_P, |P| - c_P) >= min_mac, reported in site order.
 * Classes at core k: K = 1: class a = the members of P whose bit at k is a; K = 2: class 0 = A, class 1 = B.  n_g = the size,
 * C_g = n_g (n_g - 1) / 2.  Half 0 walks towards lower coordinates, half 1 towards higher; x_j = the ordinal j steps from k.
 * surv(j) = the pairs of class g identical at every stepped site from x_j to k, k included (K = 1: surv(0) = C_g; K = 2: the
 * pairs that agree at k).  Reach J: the largest j for which x_j exists and, for the base-pair measure, |p(x_j) - p(k)| <=
 * max_extend_bp when that is non-zero, for the site measure, j <= max_extend_sites when that is non-zero.  Stop j*: the largest
 * j <= J with 1000 surv(j) >= cutoff_milli C_g.  If that fails at j = 0, or n_g < 2, the integral is 0 and no flag is set.
 *   ihh2[g][h] = sum over j < j* of (surv(j) + surv(j+1)) |p(x_j+1) - p(x_j)|      (twice the trapezoid, base pairs)
 *   sl2[g][h]  = sum over j < j* of (surv(j) + surv(j+1))                           (the same in sites)
 * Flags, bit 4 measure + 2 g + h (measure 0 = base pairs, 1 = sites): EDGE (bits 0..7) when j* = J and every existing x_j was
 * within the limit, LIMIT (bits 8..15) when j* = J and the limit set J.  Either means the cutoff was not reached.
 * Host doubles: iHH_g = (ihh2[g][0] + ihh2[g][1]) / (2 C_g), SL_g likewise; iHS = ln(iHH_1 / iHH_0), XP-EHH = ln(iHH_A / iHH_B).
 * Capacity: *n_cores always receives the number of cores.  Records are written only when out_host is non-NULL and capacity is
 * at least that number; else the call returns IMPOP_OK after the classification alone.
 * Known answer: rows over 7 sites, site 0 first, h0 = 1011010, h1 = 1011000, h2 = 0011010, h3 = 0100110, h4 = 0101110,
 * h5 = 1101100; all haplotypes, the whole matrix, min_mac 3, cutoff_milli 300, no limits.  Stepped: sites 0..5.  Four cores
 * (site: n, c1, flags, ihh2 = sl2 as [[g0h0, g0h1], [g1h0, g1h1]]):
 *   0: (3,3) (0,3)  85 [[0,6],[0,10]]     1: (3,3) (0,3) 119 [[4,22],[4,12]]
 *   2: (3,3) (0,3) 221 [[10,6],[10,16]]   4: (3,3) (0,3) 187 [[22,4],[8,4]]
 * With max_extend_bp 2 and max_extend_sites 1 the same cores give flags 43605, 43605, 64005, 21930,
 * ihh2 [[0,6],[0,6]], [[4,12],[4,10]], [[10,6],[10,12]], [[12,4],[6,4]] and sl2 [[0,4],[0,4]], [[4,6],[4,6]], [[6,4],[6,6]],
 * [[6,4],[4,4]].
 * A wrong struct_size, min_mac == 0, cutoff_milli > 1000, a site range that is empty or outside the matrix (or 2^32 sites long),
 * a core range outside the site range, overlapping populations, a population of fewer than 2 members and mask_b without mask_a
 * return IMPOP_E_INVALID; |P| > IMPOP_IHS_SCAN_MAX_N IMPOP_E_UNSUPPORTED; all before anything is uploaded or launched.
 * Chunks: the walk is cut into chunks of 64-site blocks, each warmed up from the farthest site its cores may reach under either
 * limit.  The default length makes the warm-up a minor share of a chunk's steps.  A measure without a limit reaches the end of
 * the range, so with either limit 0 there is one chunk per direction: exact, and slow on a long range.
 * IMPOP_IHS_CHUNK_BLOCKS=n (1..4096) sets the chunk length (a test aid); records never change with it.
 * Under IMPOP_TRACE=1 a call that gets past its refusals prints one line on stderr:
 *   [impop_ihs_scan] route=<dense|compact> pops= members= stepped= cores= chunks= warmup_steps= launches= bytes_streamed=
 * (chunks, warmup_steps: 0 when only the count was asked for; bytes_streamed: the rows the classification and the walks read). */
typedef struct impop_ihs_params {        /* 32 bytes */
    uint32_t struct_size;
    uint32_t min_mac;                    /* >= 1 */
    uint32_t cutoff_milli;               /* 0..1000: EHH cutoff in thousandths */
    uint32_t reserved;
    uint64_t max_extend_bp;              /* 0 = none */
    uint64_t max_extend_sites;           /* 0 = none */
} impop_ihs_params;
typedef struct impop_ihs_core {          /* 96 bytes, fixed layout, all integers */
    uint64_t site;
    uint32_t n[2];                       /* class sizes */
    uint32_t c1[2];                      /* carriers of allele 1 in each class */
    uint32_t flags;
    uint32_t reserved;
    uint64_t ihh2[2][2];                 /* [class][half] */
    uint64_t sl2[2][2];
} impop_ihs_core;
int impop_ihs_scan(impop_ctx *ctx, const impop_matrix *m, uint64_t site_begin, uint64_t site_end, uint64_t core_begin,
                   uint64_t core_end, const uint64_t *mask_a, const uint64_t *mask_b, const impop_ihs_params *params,
                   impop_ihs_core *out_host /* nullable */, uint64_t capacity, uint64_t *n_cores);
/* With impop_ctx_gram_timing on, impop_ihs_scan brackets its kernels: kernel_ms[0] = classification, prefix and tables,
 * [1] = the walk, summed since enable / reset; calls = walks timed. */
int impop_ctx_ihs_elapsed(impop_ctx *ctx, double kernel_ms[2], uint64_t *calls);
#ifdef __cplusplus
}
#endif
#endif /* IMPOP_HIP_H */
