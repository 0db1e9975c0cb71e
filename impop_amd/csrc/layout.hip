// layout.hip — presence-matrix residency: upload, SB64 <-> hap-major transposition on the
// device (wave64 readlane / ballot bit transposes), the synthetic generator and download.
#include <string.h>

#include <algorithm>
#include <vector>

#include "device_utils.h"
#include "internal.h"
#include "sb64.h"

namespace impop {

static SbGeom make_geom(uint32_t n_hap, uint64_t n_site) {
    SbGeom g;
    g.n_hap = n_hap;
    g.wps = (n_hap + 31) / 32;
    g.G = (g.wps + 3) / 4;
    g.r = g.wps - 4 * (g.G - 1);
    g.n_site = n_site;
    g.n_block = (n_site + 63) / 64;
    return g;
}

// The index's share of a kernel that writes SB64, one wave per block and lane = site: c of the lane's n_hap haplotypes carry
// its site (live: the site exists).  One ballot per wanted class; lane 0 stores the mask and its popcount.
__device__ inline void class_ballots(const ClassOut &o, bool live, uint32_t c, uint32_t n_hap, uint64_t b, uint32_t lane) {
    const bool in[N_CLASS] = {c > 0 && c < n_hap, c > IMPOP_RARE_MAX && n_hap - c > IMPOP_RARE_MAX, c == 1 || n_hap - c == 1};
#pragma unroll
    for (int k = 0; k < N_CLASS; ++k)
        if (o.mask[k]) {
            const uint64_t v = __ballot(live && in[k]);
            if (lane == 0) { o.mask[k][b] = v; o.cnt[k][b] = (uint32_t)__popcll(v); }
        }
}

// ---- hap-major -> SB64 --------------------------------------------------------------
// One wave per 64-site block.  For each 32-haplotype dword k, lanes 0..31 fetch the
// 64-site word of haplotype 32k+lane; v_readlane broadcasts each of them and every lane
// (= site) picks its own bit: a 32x64 bit transpose in 32 readlane+bfe+lshl_or steps.
// idx: the scan index's masks and counts (class_ballots).
__global__ __launch_bounds__(256) void hm_to_sb_kernel(const uint32_t *__restrict__ hm, uint64_t hm_stride,
                                                       uint32_t n_rows, uint32_t wps, uint32_t G, uint32_t r,
                                                       uint64_t n_block, uint32_t *__restrict__ sb, uint64_t n_site,
                                                       uint32_t n_hap, ClassOut idx) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t b = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= n_block) return;  // wave-uniform
    uint32_t c = 0;
    for (uint32_t k = 0; k < wps; ++k) {
        uint64_t w = 0;
        const uint32_t row = 32 * k + lane;
        if (lane < 32 && row < n_rows) {
            const uint32_t *p = hm + (uint64_t)row * hm_stride + 2 * b;
            w = (uint64_t)p[0] | ((uint64_t)p[1] << 32);
        }
        uint32_t out = 0;
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            const uint64_t wj = __shfl(w, j, 64);
            out |= (uint32_t)((wj >> lane) & 1ull) << j;
        }
        sb[sb_index(wps, G, r, b, lane, k)] = out;
        c += __popc(out);
    }
    class_ballots(idx, b * 64 + lane < n_site, c, n_hap, b, lane);
}

// ---- SB64 -> hap-major ---------------------------------------------------------------
// One wave per block; lane = site.  The 64-site hap-major word of haplotype 32k+j is bit j of every site's dword k,
// gathered by transposing the two 32 x 32 bit matrices a dword k forms over the wave's halves (below).
// phi_row != 0xFFFFFFFF (RB32 operand of the all-pairs path only): MINOR-ALLELE POLARITY.  A site more than half of the n_hap
// haplotypes carry is stored complemented, and the set of complemented sites is stored as one more row — row phi_row = n_hap, in
// the padding up to the next multiple of 96 — so that the Gram kernel delivers, for free, what undoes it:
//     I_ij = I'_ij + I'_pp - I'_ip - I'_jp      (p = phi_row; primes = the stored polarity; gram_unflip_kernel, pairwise.hip)
// while the Hamming distance a_i + a_j - 2 I_ij — all the `match` identity needs — is the same in either polarity.  Why: the FP4
// matrix cores are power-limited and their power depends on the operands (tools/micro/fp4_power_probe.hip: 4.0-4.5 PMAC/s sustained
// at 50 % ones, 4.8-4.9 at 5 % or 0 %); a presence matrix is 50 % ones only by the accident of which allele was called 1.  Measured on
// the bench matrix (ancestral polarity random): Gram 8.0 -> 7.0 ms per 4096 windows of 465 x 50 kb.
__global__ __launch_bounds__(256) void sb_to_hm_kernel(const uint32_t *__restrict__ sb, uint32_t wps, uint32_t G,
                                                       uint32_t r, uint64_t blk_begin, uint64_t blk_end,
                                                       uint32_t *__restrict__ hm, uint64_t hm_stride,
                                                       uint32_t n_rows, uint64_t rb_nb, uint32_t phi_row, uint32_t n_hap) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t b = blk_begin + (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= blk_end) return;  // wave-uniform
    uint32_t flip = 0;  // all ones: this lane's site is stored complemented
    if (phi_row != 0xFFFFFFFFu) {
        uint32_t c = 0;
        for (uint32_t k = 0; k < wps; ++k) c += (uint32_t)__popc(sb[sb_index(wps, G, r, b, lane, k)]);
        flip = 2 * c > n_hap ? 0xFFFFFFFFu : 0u;
    }
    // Dword k of site `lane` holds haplotypes 32k .. 32k+31: each half of the wave is a 32 x 32 bit matrix (site x haplotype)
    // to transpose.  Five rounds of swapping the off-diagonal s x s blocks of every 2s x 2s block with lane ^ s (s = 16 .. 1):
    // one cross-lane move + four bit operations per round, against 32 ballots per dword before (18.8 ms per 12 GB matrix;
    // 10.8 ms with the butterfly and whole-granule loads).  Afterwards lane j of half h holds, for haplotype 32k + j, the
    // sites 32h .. 32h+31 of the block: dword h of that row's pair.
    const uint32_t half = lane >> 5, j = lane & 31;
    const uint32_t *blk = sb + b * 64ull * wps;
    uint4 q = {0u, 0u, 0u, 0u};  // the granule dword k comes out of
    for (uint32_t k = 0; k < wps; ++k) {
        // whole granules as one 16-byte load per lane (dword k alone is a 4-byte read at a 16-byte stride: a quarter of
        // every cache line per instruction); the last, shorter granule dword by dword
        uint32_t w;
        if ((k >> 2) + 1 < G || r == 4) {
            static_assert(sizeof(uint4) == 16, "granule");
            if ((k & 3) == 0) q = *reinterpret_cast<const uint4 *>(blk + (uint64_t)(k >> 2) * 256 + lane * 4);
            w = (k & 3) == 0 ? q.x : (k & 3) == 1 ? q.y : (k & 3) == 2 ? q.z : q.w;
        } else {
            w = sb[sb_index(wps, G, r, b, lane, k)];
        }
        if (flip) w ^= 32 * k + 32 <= n_hap ? 0xFFFFFFFFu : 32 * k < n_hap ? (1u << (n_hap - 32 * k)) - 1u : 0u;  // real haplotypes only
#pragma unroll
        for (uint32_t s = 16; s != 0; s >>= 1) {
            const uint32_t M = s == 16 ? 0x0000FFFFu : s == 8 ? 0x00FF00FFu : s == 4 ? 0x0F0F0F0Fu : s == 2 ? 0x33333333u : 0x55555555u;
            const uint32_t o = (uint32_t)__shfl_xor((int)w, (int)s, 64);
            w = (lane & s) ? ((w & ~M) | ((o >> s) & M)) : ((w & M) | ((o & M) << s));
        }
        const uint32_t row = 32 * k + j;
        if (row < n_rows && row != phi_row) {
            const uint64_t d = 2 * (b - blk_begin);  // first of the two dwords of this 64-site block
            uint32_t *p = rb_nb ? hm + ((((uint64_t)(row >> 5) * rb_nb + (d >> 1)) * 32 + (row & 31)) * 2)
                                : hm + (uint64_t)row * hm_stride + d;
            p[half] = w;
        }
    }
    if (phi_row != 0xFFFFFFFFu) {  // the complemented sites of this block as the 64-site word of row phi_row
        const uint64_t bal = __ballot(flip != 0);
        if (j == 0) {
            const uint64_t d = 2 * (b - blk_begin);
            uint32_t *p = hm + ((((uint64_t)(phi_row >> 5) * rb_nb + (d >> 1)) * 32 + (phi_row & 31)) * 2);
            p[half] = half ? (uint32_t)(bal >> 32) : (uint32_t)bal;
        }
    }
}

// zero the bits of sites >= n_site in the last used dword pair of every hap-major row
__global__ void hm_clear_tail_kernel(uint32_t *hm, uint64_t hm_stride, uint32_t n_rows, uint64_t n_site,
                                     uint64_t n_dwords_used) {
    const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n_rows) return;
    uint32_t *p = hm + (uint64_t)row * hm_stride;
    const uint64_t first = n_site >> 5;
    if (first < n_dwords_used) {
        const uint32_t keepbits = (uint32_t)(n_site & 31);
        p[first] &= keepbits ? ((1u << keepbits) - 1u) : 0u;
        for (uint64_t d = first + 1; d < n_dwords_used; ++d) p[d] = 0;
    }
}

int launch_hm_to_sb(impop_ctx *ctx, const uint32_t *d_hm, uint64_t hm_stride, const SbGeom &g, uint32_t *d_sb, const ClassOut &idx) {
    if (g.n_block == 0) return IMPOP_OK;
    const uint64_t grid = (g.n_block + 3) / 4;
    REQUIRE(grid < 0x7FFFFFFFull, "matrix too long for one launch (%llu blocks)", (unsigned long long)g.n_block);
    const uint32_t n_rows = (g.n_hap + 95) / 96 * 96;
    hipLaunchKernelGGL(hm_to_sb_kernel, dim3((uint32_t)grid), dim3(256), 0, ctx->stream, d_hm, hm_stride, n_rows, g.wps,
                       g.G, g.r, g.n_block, d_sb, g.n_site, g.n_hap, idx);
    HIP_TRY(hipGetLastError());
    return IMPOP_OK;
}

int launch_sb_to_hm(impop_ctx *ctx, const uint32_t *d_sb, const SbGeom &g, uint64_t blk_begin, uint64_t blk_end,
                    uint32_t *d_hm, uint64_t hm_stride, uint32_t n_rows, uint64_t rb_nb, uint32_t phi_row) {
    if (blk_end <= blk_begin) return IMPOP_OK;
    REQUIRE(phi_row == 0xFFFFFFFFu || (rb_nb != 0 && phi_row == g.n_hap && phi_row < n_rows), "launch_sb_to_hm: bad phi_row");
    const uint64_t grid = (blk_end - blk_begin + 3) / 4;
    REQUIRE(grid < 0x7FFFFFFFull, "range too long for one launch");
    hipLaunchKernelGGL(sb_to_hm_kernel, dim3((uint32_t)grid), dim3(256), 0, ctx->stream, d_sb, g.wps, g.G, g.r, blk_begin,
                       blk_end, d_hm, hm_stride, n_rows, rb_nb, phi_row, g.n_hap);
    HIP_TRY(hipGetLastError());
    return IMPOP_OK;
}

// ---- synthetic generator ---------------------------------------------------------------
struct SynthDev {
    uint64_t seed;
    uint32_t n_founder;
    uint32_t thr_founder;  // p_founder * 2^32
    uint32_t thr_private;  // p_private_word * 2^32
};

// tables: fmask[f*wps + k] (haplotypes of founder f in dword k), then valid[k]
__global__ __launch_bounds__(256) void synth_sb_kernel(SynthDev p, const uint32_t *__restrict__ tables, uint32_t wps,
                                                       uint32_t G, uint32_t r, uint64_t n_block, uint64_t n_site,
                                                       uint64_t site0, uint32_t *__restrict__ sb, uint32_t n_hap, ClassOut idx) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t b = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= n_block) return;
    const bool live = b * 64 + lane < n_site;
    const uint64_t s = site0 + b * 64 + lane;  // the generator is counter-based on the GLOBAL site index: a slab is a cut of the whole
#ifdef IMPOP_SYNTH_ANC0  // experiment builds only (tools/): every ancestral allele 0 => a sparse matrix with the same pairwise distances
    const uint32_t anc = 0u;
#else
    const uint32_t anc = (synth_hash(p.seed, 1, s) & 1ull) ? 0xFFFFFFFFu : 0u;
#endif
    uint32_t fl = 0;
    for (uint32_t f = 0; f < p.n_founder; ++f)
        if ((uint32_t)(synth_hash(p.seed, 2 + f, s) >> 32) < p.thr_founder) fl |= 1u << f;
    const uint32_t *valid = tables + (uint64_t)p.n_founder * wps;
    uint32_t c = 0;  // carriers of this lane's site: the scan index's masks come from ballots, not from a second pass
    for (uint32_t k = 0; k < wps; ++k) {
        uint32_t w = anc;
        uint32_t m = fl;
        while (m) {
            const int f = __ffs(m) - 1;
            m &= m - 1;
            w ^= tables[(uint64_t)f * wps + k];
        }
        const uint64_t h = synth_hash(p.seed, 64 + k, s);
        if ((uint32_t)(h >> 32) < p.thr_private) w ^= 1u << (uint32_t)(h & 31);
        w = live ? w & valid[k] : 0u;
        c += __popc(w);
        sb[sb_index(wps, G, r, b, lane, k)] = w;
    }
    class_ballots(idx, live, c, n_hap, b, lane);
}

static int alloc_matrix(impop_ctx *ctx, uint32_t n_hap, uint64_t n_site, bool want_hm, impop_matrix **out) {
    impop_matrix *m = new impop_matrix();
    m->g = make_geom(n_hap, n_site);
    m->device = ctx->device;
    m->n_hap_pad = (n_hap + 95) / 96 * 96;  // Gram tiles are 96 haplotypes wide (3 row groups of 32)
    {   // minor-allele polarity of the all-pairs operand (sb_to_hm_kernel) needs one padding row for the set of complemented sites
        static const bool off = env_is("IMPOP_NO_POLARITY", '1');
        m->phi_row = (want_hm && !off && n_hap % 96 != 0 && n_hap <= 16384 /* gram_unflip_kernel's LDS */) ? n_hap : 0xFFFFFFFFu;
    }
    m->sb_bytes = m->g.n_block * 64ull * m->g.wps * 4ull;
    // one extra block of slack so software-pipelined kernels may prefetch one block past the end
    hipError_t e = hipMalloc((void **)&m->d_sb, m->sb_bytes + 64ull * m->g.wps * 4ull + 256);
    if (e != hipSuccess) {
        delete m;
        return hip_fail(e, "hipMalloc(SB64 matrix)", __FILE__, __LINE__);
    }
    e = hipMemsetAsync((char *)m->d_sb + m->sb_bytes, 0, 64ull * m->g.wps * 4ull + 256, ctx->stream);
    if (e != hipSuccess) {
        hipFree(m->d_sb);
        delete m;
        return hip_fail(e, "hipMemsetAsync", __FILE__, __LINE__);
    }
    if (want_hm) {
        m->rb_nb = m->g.n_block + 8;  // 64-site cells per row group + slack (a 4-cell Gram step may overhang the last cell)
        m->rb_bytes = (uint64_t)(m->n_hap_pad / 32) * m->rb_nb * 32ull * 8ull;
        e = hipMalloc((void **)&m->d_rb, m->rb_bytes);
        if (e != hipSuccess) {
            hipFree(m->d_sb);
            delete m;
            return hip_fail(e, "hipMalloc(row-group-blocked matrix)", __FILE__, __LINE__);
        }
        e = hipMemsetAsync(m->d_rb, 0, m->rb_bytes, ctx->stream);
        if (e != hipSuccess) {
            hipFree(m->d_sb);
            hipFree(m->d_rb);
            delete m;
            return hip_fail(e, "hipMemsetAsync", __FILE__, __LINE__);
        }
    }
    *out = m;
    return IMPOP_OK;
}

// variable-site scan index (built below, next to the compaction kernels it shares): index_begin allocates the per-block mask
// and prefix (or records why there is none), the kernel that writes SB64 fills the mask by ballot, index_finish does the rest
struct IndexBuild {
    ClassOut out;               // per class wanted: its mask (== m->idx[k].mask while the build goes on) and its counts (inside d_tmp)
    uint32_t n_class = 0;       // the classes wanted: KEPT .. n_class - 1
    void *d_tmp = nullptr;      // transient: counts, chunk sums, totals (IndexTmp)
    uint64_t *d_pos = nullptr;  // transient: source site of every kept site
    uint64_t n_chunks = 0;
    uint32_t keep_flags = 0;    // the caller's, for what index_finish builds on top (unique_rows_build)
    IndexBuild() = default;
    IndexBuild(const IndexBuild &) = delete;
    ~IndexBuild() {
        if (d_tmp) hipFree(d_tmp);
        if (d_pos) hipFree(d_pos);
    }
};
static int index_begin(impop_ctx *ctx, impop_matrix *m, uint32_t keep_flags, IndexBuild &ib);
static int index_finish(impop_ctx *ctx, impop_matrix *m, IndexBuild &ib);

}  // namespace impop

using namespace impop;

IMPOP_API int impop_matrix_upload(impop_ctx *ctx, const uint64_t *bits, uint32_t n_hap, uint64_t n_site,
                                  uint64_t row_stride_words, uint32_t keep_flags, impop_matrix **out) {
    REQUIRE(ctx && out, "impop_matrix_upload: ctx/out is NULL");
    *out = nullptr;
    REQUIRE(n_hap >= 1, "impop_matrix_upload: n_hap must be >= 1");
    REQUIRE(n_hap <= (1u << 20), "impop_matrix_upload: n_hap %u too large", n_hap);
    const uint64_t words = (n_site + 63) / 64;
    REQUIRE(n_site == 0 || bits, "impop_matrix_upload: bits is NULL");
    REQUIRE(row_stride_words >= words, "impop_matrix_upload: row_stride_words %llu < ceil(n_site/64) = %llu",
            (unsigned long long)row_stride_words, (unsigned long long)words);
    HIP_TRY(hipSetDevice(ctx->device));
    impop_matrix *m = nullptr;
    const bool want_rb = (keep_flags & IMPOP_KEEP_HAP_MAJOR) != 0;
    int rc = alloc_matrix(ctx, n_hap, n_site, want_rb, &m);
    if (rc) return rc;
    // transient plain hap-major staging copy of the caller's rows (freed before returning)
    const uint64_t hm_stride = std::max<uint64_t>((m->g.n_block * 2 + 3) / 4 * 4, 4);
    const uint64_t hm_bytes = (uint64_t)m->n_hap_pad * hm_stride * 4ull;
    uint32_t *d_hm = nullptr;
    auto fail = [&](int code) {
        if (d_hm) hipFree(d_hm);
        impop_matrix_free(ctx, m);
        return code;
    };
    hipError_t e = hipMalloc((void **)&d_hm, hm_bytes);
    if (e != hipSuccess) return fail(hip_fail(e, "hipMalloc(upload staging)", __FILE__, __LINE__));
    e = hipMemsetAsync(d_hm, 0, hm_bytes, ctx->stream);
    if (e != hipSuccess) return fail(hip_fail(e, "hipMemsetAsync", __FILE__, __LINE__));
    if (words) {
        e = hipMemcpy2DAsync(d_hm, hm_stride * 4ull, bits, row_stride_words * 8ull, words * 8ull, n_hap,
                             hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) return fail(hip_fail(e, "hipMemcpy2DAsync(upload)", __FILE__, __LINE__));
        hipLaunchKernelGGL(hm_clear_tail_kernel, dim3((m->n_hap_pad + 255) / 256), dim3(256), 0, ctx->stream, d_hm, hm_stride,
                           m->n_hap_pad, n_site, words * 2);
        if ((e = hipGetLastError()) != hipSuccess) return fail(hip_fail(e, "hm_clear_tail_kernel", __FILE__, __LINE__));
    }
    IndexBuild ib;
    rc = index_begin(ctx, m, keep_flags, ib);
    if (rc) return fail(rc);
    rc = launch_hm_to_sb(ctx, d_hm, hm_stride, m->g, m->d_sb, ib.out);
    if (rc) return fail(rc);
    rc = index_finish(ctx, m, ib);
    if (rc) return fail(rc);
    if (want_rb) {
        rc = launch_sb_to_hm(ctx, m->d_sb, m->g, 0, m->g.n_block, m->d_rb, 0, m->n_hap_pad, m->rb_nb, m->phi_row);
        if (rc) return fail(rc);
        rc = ensure_segmap(ctx, m);  // a matrix kept for the all-pairs path gets its site bitmap (S per window) right away
        if (rc) return fail(rc);
    }
    e = hipStreamSynchronize(ctx->stream);  // the caller may free `bits` on return
    if (e != hipSuccess) return fail(hip_fail(e, "hipStreamSynchronize", __FILE__, __LINE__));
    hipFree(d_hm);
    *out = m;
    return IMPOP_OK;
}

IMPOP_API int impop_matrix_synthetic(impop_ctx *ctx, uint32_t n_hap, uint64_t n_site, const impop_synth_params *p,
                                     uint32_t keep_flags, impop_matrix **out) {
    return impop_matrix_synthetic_slab(ctx, n_hap, 0, n_site, p, keep_flags, out);
}

IMPOP_API int impop_matrix_synthetic_slab(impop_ctx *ctx, uint32_t n_hap, uint64_t site_begin, uint64_t n_site,
                                          const impop_synth_params *p, uint32_t keep_flags, impop_matrix **out) {
    REQUIRE(ctx && out && p, "impop_matrix_synthetic: NULL argument");
    *out = nullptr;
    REQUIRE(site_begin + n_site >= site_begin, "impop_matrix_synthetic_slab: site range wraps");
    REQUIRE(n_hap >= 1 && n_hap <= (1u << 20), "impop_matrix_synthetic: bad n_hap %u", n_hap);
    REQUIRE(p->n_founder >= 1 && p->n_founder <= 32, "impop_matrix_synthetic: n_founder must be 1..32");
    REQUIRE(p->p_founder >= 0 && p->p_founder < 1 && p->p_private_word >= 0 && p->p_private_word < 1,
            "impop_matrix_synthetic: probabilities must be in [0,1)");
    HIP_TRY(hipSetDevice(ctx->device));
    impop_matrix *m = nullptr;
    const bool want_hm = (keep_flags & IMPOP_KEEP_HAP_MAJOR) != 0;
    int rc = alloc_matrix(ctx, n_hap, n_site, want_hm, &m);
    if (rc) return rc;
    auto fail = [&](int code) {
        impop_matrix_free(ctx, m);
        return code;
    };
    const uint32_t wps = m->g.wps;
    std::vector<uint32_t> tables((size_t)(p->n_founder + 1) * wps, 0u);
    for (uint32_t h = 0; h < n_hap; ++h) {
        const uint32_t f = (uint32_t)(synth_hash(p->seed, 1000, h) % p->n_founder);
        tables[(size_t)f * wps + (h >> 5)] |= 1u << (h & 31);
        tables[(size_t)p->n_founder * wps + (h >> 5)] |= 1u << (h & 31);
    }
    void *d_tab = nullptr;
    rc = ctx_scratch(ctx, tables.size() * 4, &d_tab);
    if (rc) return fail(rc);
    hipError_t e = hipMemcpyAsync(d_tab, tables.data(), tables.size() * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) return fail(hip_fail(e, "hipMemcpyAsync(tables)", __FILE__, __LINE__));
    SynthDev sp;
    sp.seed = p->seed;
    sp.n_founder = p->n_founder;
    sp.thr_founder = (uint32_t)(p->p_founder * 4294967296.0);
    sp.thr_private = (uint32_t)(p->p_private_word * 4294967296.0);
    IndexBuild ib;
    rc = index_begin(ctx, m, keep_flags, ib);
    if (rc) return fail(rc);
    if (m->g.n_block) {
        const uint64_t grid = (m->g.n_block + 3) / 4;
        if (grid >= 0x7FFFFFFFull) {
            set_error("impop_matrix_synthetic: too many sites");
            return fail(IMPOP_E_INVALID);
        }
        hipLaunchKernelGGL(synth_sb_kernel, dim3((uint32_t)grid), dim3(256), 0, ctx->stream, sp, (const uint32_t *)d_tab,
                           wps, m->g.G, m->g.r, m->g.n_block, n_site, site_begin, m->d_sb, n_hap, ib.out);
        if ((e = hipGetLastError()) != hipSuccess) return fail(hip_fail(e, "synth_sb_kernel", __FILE__, __LINE__));
        if (want_hm) {
            rc = launch_sb_to_hm(ctx, m->d_sb, m->g, 0, m->g.n_block, m->d_rb, 0, m->n_hap_pad, m->rb_nb, m->phi_row);
            if (rc) return fail(rc);
            rc = ensure_segmap(ctx, m);
            if (rc) return fail(rc);
        }
    }
    rc = index_finish(ctx, m, ib);
    if (rc) return fail(rc);
    e = hipStreamSynchronize(ctx->stream);  // `tables` (pageable) must stay alive until the copy is done
    if (e != hipSuccess) return fail(hip_fail(e, "hipStreamSynchronize", __FILE__, __LINE__));
    *out = m;
    return IMPOP_OK;
}

IMPOP_API int impop_matrix_download(impop_ctx *ctx, const impop_matrix *m, uint64_t site_begin, uint64_t site_end,
                                    uint64_t *out, uint64_t row_stride_words) {
    REQUIRE(ctx && m, "impop_matrix_download: NULL argument");
    REQUIRE(site_begin <= site_end && site_end <= m->g.n_site, "impop_matrix_download: bad site range [%llu,%llu)",
            (unsigned long long)site_begin, (unsigned long long)site_end);
    const uint64_t W = site_end - site_begin;
    const uint64_t out_words = (W + 63) / 64;
    REQUIRE(row_stride_words >= out_words, "impop_matrix_download: row_stride_words too small");
    if (W == 0) return IMPOP_OK;
    REQUIRE(out, "impop_matrix_download: out is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    const uint64_t b0 = site_begin / 64, b1 = (site_end + 63) / 64;
    const uint64_t nb = b1 - b0;
    const uint64_t stride = nb * 2;  // dwords per row in the temporary
    const uint32_t n_rows = m->g.n_hap;
    void *d_tmp = nullptr;
    int rc = ctx_scratch(ctx, (size_t)n_rows * stride * 4, &d_tmp);
    if (rc) return rc;
    rc = launch_sb_to_hm(ctx, m->d_sb, m->g, b0, b1, (uint32_t *)d_tmp, stride, n_rows);
    if (rc) return rc;
    std::vector<uint64_t> tmp((size_t)n_rows * nb);
    HIP_TRY(hipMemcpyAsync(tmp.data(), d_tmp, tmp.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const uint32_t sh = (uint32_t)(site_begin & 63);
    for (uint32_t i = 0; i < n_rows; ++i) {
        const uint64_t *src = tmp.data() + (size_t)i * nb;
        uint64_t *dst = out + (size_t)i * row_stride_words;
        for (uint64_t w = 0; w < out_words; ++w) {
            uint64_t v = src[w] >> sh;
            if (sh && w + 1 < nb) v |= src[w + 1] << (64 - sh);
            dst[w] = v;
        }
        if (W & 63) dst[out_words - 1] &= (~0ull) >> (64 - (W & 63));
    }
    return IMPOP_OK;
}

// ---- compaction to the variable sites ------------------------------------------------------------
// Monomorphic sites (c_s = 0 or c_s = n over ALL haplotypes) add 0 to every sum_s c(n - c) of every
// subset and are never segregating, so the scan statistics of a window depend on its variable sites
// and its LENGTH only.  A compacted matrix keeps those sites (with their original positions) and is
// scanned with windows in the original coordinates: same records, ~W/S times fewer bytes.
namespace impop {

// grid-stride over blocks: a workgroup per 4 blocks cost more in launches than in bytes (37 ms for 14.6 GB)
__global__ __launch_bounds__(256) void variable_mask_kernel(const uint32_t *__restrict__ sb, uint32_t wps, uint32_t G,
                                                            uint32_t r, uint64_t n_block, uint64_t n_site, uint32_t n_hap,
                                                            ClassOut idx /* KEPT */, uint64_t *__restrict__ ones /* nullable: sites with c = n */) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * 4;
    for (uint64_t b = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); b < n_block; b += stride) {
        uint32_t c = 0;
        sb_for_each_dword<false>(sb + b * 64ull * wps, G, r, lane, [&](uint32_t, uint32_t w) { c += __popc(w); });
        class_ballots(idx, b * 64 + lane < n_site, c, n_hap, b, lane);
        const uint64_t o = ones ? __ballot((b * 64 + lane < n_site) && c == n_hap) : 0ull;
        if (lane == 0 && ones) ones[b] = o;
    }
}

// Two-level exclusive scan of per-block counts, up to N_CLASS arrays in one launch each (the class on grid dimension y):
// base[k][b] = the sum of cnt[k][< b], total[k] = the sum of them all.  chunk: n_chunks sums per class, class after class.
constexpr uint32_t SCAN_CHUNK = 1024;  // blocks per workgroup
struct PrefixArgs {
    const uint32_t *cnt[N_CLASS];
    uint64_t *base[N_CLASS];
};
__global__ __launch_bounds__(256) void chunk_sum_kernel(PrefixArgs a, uint64_t n, uint64_t *__restrict__ chunk_sum) {
    __shared__ uint64_t sh[4];
    const uint32_t *cnt = a.cnt[blockIdx.y];
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_CHUNK;
    uint64_t t = 0;
    for (uint32_t i = threadIdx.x; i < SCAN_CHUNK; i += 256)
        if (base + i < n) t += cnt[base + i];
    t = wave_sum_u64(t);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) chunk_sum[(uint64_t)blockIdx.y * gridDim.x + blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}
__global__ void chunk_scan_kernel(uint64_t *chunk_sum, uint64_t n_chunks, uint64_t *total) {  // one thread per class: n_chunks is small
    if (threadIdx.x) return;
    chunk_sum += blockIdx.x * n_chunks;
    uint64_t run = 0;
    for (uint64_t i = 0; i < n_chunks; ++i) {
        const uint64_t v = chunk_sum[i];
        chunk_sum[i] = run;
        run += v;
    }
    total[blockIdx.x] = run;
}
__global__ __launch_bounds__(64) void block_base_kernel(PrefixArgs a, uint64_t n, const uint64_t *__restrict__ chunk_off) {
    // one wave per chunk: 16 rounds of a 64-wide exclusive scan
    const uint32_t *cnt = a.cnt[blockIdx.y];
    uint64_t *base = a.base[blockIdx.y];
    const uint64_t b0 = (uint64_t)blockIdx.x * SCAN_CHUNK;
    uint64_t run = chunk_off[(uint64_t)blockIdx.y * gridDim.x + blockIdx.x];
    for (uint32_t rnd = 0; rnd < SCAN_CHUNK / 64; ++rnd) {
        const uint64_t i = b0 + rnd * 64 + threadIdx.x;
        const uint64_t v = i < n ? cnt[i] : 0;
        uint64_t incl = v;
        for (int off = 1; off < 64; off <<= 1) {
            const uint64_t o = __shfl_up(incl, off, 64);
            if ((int)threadIdx.x >= off) incl += o;
        }
        if (i < n) base[i] = run + incl - v;
        run += __shfl(incl, 63, 64);
    }
}
__global__ __launch_bounds__(256) void gather_variable_kernel(const uint32_t *__restrict__ sb, uint32_t wps, uint32_t G, uint32_t r,
                                                              uint64_t n_block, const uint64_t *__restrict__ mask,
                                                              const uint64_t *__restrict__ base, uint32_t *__restrict__ out,
                                                              uint64_t *__restrict__ pos) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * 4;
    for (uint64_t b = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); b < n_block; b += stride) {
        const uint64_t m = mask[b];
        if (!m) continue;  // wave-uniform: most blocks of a real matrix hold a few variable sites, many none
        if (!((m >> lane) & 1ull)) continue;
        const uint64_t dest = base[b] + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
        for (uint32_t k = 0; k < wps; ++k)
            out[sb_index(wps, G, r, dest >> 6, (uint32_t)(dest & 63), k)] = sb[sb_index(wps, G, r, b, lane, k)];
        pos[dest] = b * 64 + lane;
    }
}

// Two levels: a binary search over 10^7 positions (87 MB) misses the cache on nearly every step — 8192 window edges cost
// 0.7-4 ms per call, as much as the Gram launch they precede; every 4096th position (a few thousand entries, cache
// resident) narrows the search to one 32 KB run first.
__global__ void map_edges_kernel(const uint64_t *__restrict__ pos, uint64_t n_pos, const impop_window *__restrict__ win, uint64_t n_win,
                                 impop_window *__restrict__ out) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 2 * n_win) return;
    const uint64_t key = (e & 1) ? win[e >> 1].site_end : win[e >> 1].site_begin;
    uint64_t lo = 0, len = n_pos;  // first kept site at or right of `key` (= kept sites left of it)
    while (len) {
        const uint64_t half = len >> 1;
        if (pos[lo + half] < key) { lo += half + 1; len -= half + 1; }
        else len = half;
    }
    if (e & 1) out[e >> 1].site_end = lo;
    else { out[e >> 1].site_begin = lo; out[e >> 1].seq_len = win[e >> 1].seq_len; }
}

int map_windows_device(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n, std::vector<impop_window> &mapped) {
    if (!m->compact || !m->d_pos || n < 256) {  // few windows: the host search is quicker than a launch and two copies
        map_windows(m, windows, n, mapped);
        return IMPOP_OK;
    }
    REQUIRE((2 * n + 255) / 256 < 0x7FFFFFFFull, "map_windows_device: too many windows");
    void *d = nullptr;
    const int rc = ctx_aux(ctx, 0, 2 * n * sizeof(impop_window), &d);  // slot 0 (h-fst partials) is idle before the first launch of a call
    if (rc) return rc;
    impop_window *d_in = reinterpret_cast<impop_window *>(d), *d_out = d_in + n;
    mapped.resize(n);
    HIP_TRY(hipMemcpyAsync(d_in, windows, n * sizeof(impop_window), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(map_edges_kernel, dim3((uint32_t)((2 * n + 255) / 256)), dim3(256), 0, ctx->stream, m->d_pos, (uint64_t)m->pos.size(),
                       d_in, n, d_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(mapped.data(), d_out, n * sizeof(impop_window), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return IMPOP_OK;
}

uint64_t pos_lower_bound(const impop_matrix *m, uint64_t s) {
    const std::vector<uint64_t> &pos = m->pos, &co = m->pos_coarse;
    if (co.empty()) return (uint64_t)(std::lower_bound(pos.begin(), pos.end(), s) - pos.begin());
    // first coarse entry >= s: the answer lies in (its predecessor's index, its index]
    const size_t c = (size_t)(std::lower_bound(co.begin(), co.end(), s) - co.begin());
    const size_t lo = c == 0 ? 0 : ((c - 1) << POS_COARSE_SHIFT) + 1;
    const size_t hi = c < co.size() ? (c << POS_COARSE_SHIFT) : pos.size();
    return (uint64_t)(std::lower_bound(pos.begin() + lo, pos.begin() + hi, s) - pos.begin());
}

// The window edges of a batch, 32 searches in lock step: after the coarse level every search is a dozen DEPENDENT cache
// misses in its own 32 KB run (250 ns per edge one after the other: 2 ms per 4096 windows, as long as the Gram launch that
// follows); interleaved, the misses of different edges overlap, and each step's next probe is prefetched while the other
// edges take theirs.
void map_windows(const impop_matrix *m, const impop_window *windows, uint64_t n, std::vector<impop_window> &mapped) {
    mapped.assign(windows, windows + n);
    if (!m->compact) return;
    const uint64_t *pos = m->pos.data();
    const std::vector<uint64_t> &co = m->pos_coarse;
    constexpr int Q = 32;
    uint64_t key[Q];
    size_t base[Q], len[Q];
    for (uint64_t i0 = 0; i0 < 2 * n; i0 += Q) {
        const int cnt = (int)std::min<uint64_t>(Q, 2 * n - i0);
        for (int q = 0; q < cnt; ++q) {
            const uint64_t e = i0 + q;
            key[q] = (e & 1) ? windows[e >> 1].site_end : windows[e >> 1].site_begin;
            size_t lo = 0, hi = m->pos.size();
            if (!co.empty()) {  // first coarse entry >= key: the answer lies in (its predecessor's index, its index]
                const size_t c = (size_t)(std::lower_bound(co.begin(), co.end(), key[q]) - co.begin());
                lo = c == 0 ? 0 : ((c - 1) << POS_COARSE_SHIFT) + 1;
                hi = c < co.size() ? (c << POS_COARSE_SHIFT) : m->pos.size();
            }
            base[q] = lo;
            len[q] = hi - lo;
            if (len[q]) __builtin_prefetch(pos + lo + (len[q] >> 1));
        }
        for (bool more = true; more;) {
            more = false;
            for (int q = 0; q < cnt; ++q) {
                if (!len[q]) continue;
                const size_t half = len[q] >> 1;
                if (pos[base[q] + half] < key[q]) {
                    base[q] += half + 1;
                    len[q] -= half + 1;
                } else {
                    len[q] = half;
                }
                if (len[q]) {
                    __builtin_prefetch(pos + base[q] + (len[q] >> 1));
                    more = true;
                }
            }
        }
        for (int q = 0; q < cnt; ++q) {
            const uint64_t e = i0 + q;
            if (e & 1) mapped[e >> 1].site_end = base[q];
            else mapped[e >> 1].site_begin = base[q];
        }
    }
}

// ---- variable-site scan index -------------------------------------------------------------------
// The same sites impop_matrix_compact keeps, but as a second layout of the SAME matrix: windows stay in matrix coordinates,
// an edge s maps to kept(s) = base[s >> 6] + popc(mask[s >> 6] & ((1 << (s & 63)) - 1)) with no search, and every scan plan
// of an unweighted matrix streams the kept sites only (scan.hip).  A monomorphic site adds 0 to every sum c (n - c) of
// every subset and segregates in none, so the records are those of the dense stream.

// source site of every kept site (thread per source block; a block holds few kept sites, most hold none)
__global__ __launch_bounds__(256) void kept_pos_kernel(const uint64_t *__restrict__ mask, const uint64_t *__restrict__ base,
                                                       uint64_t n_block, uint64_t *__restrict__ pos) {
    const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= n_block) return;
    uint64_t v = mask[b], d = base[b];
    while (v) {
        pos[d++] = b * 64 + (uint64_t)__builtin_ctzll(v);
        v &= v - 1;
    }
}

// Destination-ordered gather: one wave per kept-site block, lane l = kept site 64j + l reads its source site's 16-byte
// granules and the wave writes each granule of the compacted block as one coalesced 1 KiB store (the last, shorter granule
// as r contiguous dwords per lane).  Lanes past n_kept write zeros: the last block is padded like any SB64 block.
__global__ __launch_bounds__(256) void gather_kept_kernel(const uint32_t *__restrict__ sb, uint32_t wps, uint32_t G, uint32_t r,
                                                          const uint64_t *__restrict__ pos, uint64_t n_kept, uint64_t n_vblock,
                                                          uint32_t *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t j = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= n_vblock) return;  // wave-uniform
    const uint64_t d = j * 64 + lane;
    const bool live = d < n_kept;
    const uint64_t s = live ? pos[d] : 0;
    const uint32_t *src = sb + (s >> 6) * 64ull * wps;
    const uint32_t sl = (uint32_t)(s & 63);
    uint32_t *dst = out + j * 64ull * wps;
    const uint32_t Gf = sb_full_granules(G, r);
    uint32_t tl[3] = {0u, 0u, 0u};
    if (live) sb_load_tail<false>(src, G, r, sl, tl);
#pragma unroll 4
    for (uint32_t g = 0; g < Gf; ++g) {
        u32v4 v = {0u, 0u, 0u, 0u};
        if (live) v = *sb_granule(src, g, sl);
        *sb_granule(dst, g, lane) = v;
    }
    uint32_t *last = sb_tail(dst, G, r, lane);
    sb_use_tail(G, r, tl, [&](uint32_t k, uint32_t w) { last[k & 3] = w; });  // k & 3: the dword's place in its granule
}

// Rare kept sites -> 8-byte entries (layout: internal.h, d_vrare).  One thread per source block walks its rare sites (a few per
// block) and reads each one's wps dwords twice: the count picks the allele to list, then the first (at most three) carriers of it.
// Singleton stream (rk has the SINGLE class): the same pass also writes every rare site to one of the two packed streams, a singleton
// as its carrier's 16 bits to out_single, any other as its entry to out_multi (internal.h, d_vsingle / d_vmulti).
__global__ __launch_bounds__(256) void rare_entries_kernel(const uint32_t *__restrict__ sb, uint32_t wps, uint32_t G, uint32_t r,
                                                           uint32_t n_hap, ClassRanks rk, uint64_t n_block, uint64_t *__restrict__ out,
                                                           uint16_t *__restrict__ out_single, uint64_t *__restrict__ out_multi) {
    const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= n_block) return;
    const bool single = rk.k[SINGLE].mask != nullptr;
    uint64_t v = rk.k[KEPT].mask[b] & ~rk.k[COMMON].mask[b], d = rk.k[KEPT].base[b] - rk.k[COMMON].base[b];
    const uint64_t sm = single ? rk.k[SINGLE].mask[b] : 0ull;
    uint64_t ds = single ? rk.k[SINGLE].base[b] : 0ull, dm = d - ds;
    while (v) {
        const uint32_t l = (uint32_t)__builtin_ctzll(v);
        v &= v - 1;
        uint32_t c = 0;
        for (uint32_t k = 0; k < wps; ++k) c += __popc(sb[sb_index(wps, G, r, b, l, k)]);
        const bool zeros = 2 * c > n_hap;  // list the carriers of 0 (padding haplotypes excluded below)
        uint64_t slots = RARE_NO_SLOTS;
        uint32_t m = 0;
        for (uint32_t k = 0; k < wps && m < IMPOP_RARE_MAX; ++k) {
            uint32_t w = sb[sb_index(wps, G, r, b, l, k)];
            if (zeros) w = ~w & (32 * k + 32 <= n_hap ? 0xFFFFFFFFu : (1u << (n_hap - 32 * k)) - 1u);
            while (w && m < IMPOP_RARE_MAX) {
                const uint32_t h = 32 * k + (uint32_t)__builtin_ctz(w);
                w &= w - 1;
                slots = rare_set_slot(slots, m++, h);
            }
        }
        const uint64_t e = rare_pack(slots, m, zeros);
        out[d++] = e;
        if (single) {
            if ((sm >> l) & 1ull) out_single[ds++] = (uint16_t)(rare_slot(e, 0) | (zeros ? 0x8000u : 0u));
            else out_multi[dm++] = e;
        }
    }
}

// window edge s -> its place in every stream of the route (tile_cut.h, EdgeCut): the ranks of the classes rk names
__global__ void map_edges_index_kernel(ClassRanks rk, const impop_window *__restrict__ win, uint64_t n_win, LayoutWindow *__restrict__ out) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 2 * n_win) return;
    const uint64_t key = (e & 1) ? win[e >> 1].site_end : win[e >> 1].site_begin;  // <= n_site: entry n_block exists
    uint64_t n[N_CLASS];
#pragma unroll
    for (int k = 0; k < N_CLASS; ++k) n[k] = rk.k[k].mask ? rk.k[k](key) : 0;
    // unsplit: the kept sites; split: the common sites, rare(s) = kept(s) - common(s) less the singletons, the singletons
    const EdgeCut c = rk.k[COMMON].mask ? EdgeCut{n[COMMON], n[KEPT] - n[COMMON] - n[SINGLE], n[SINGLE]} : EdgeCut{n[KEPT], 0, 0};
    if (e & 1) out[e >> 1].hi = c;
    else { out[e >> 1].lo = c; out[e >> 1].seq_len = win[e >> 1].seq_len; }
}

int map_windows_index(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n, SiteClass top,
                      std::vector<LayoutWindow> &out) {
    out.resize(n);
    if (!n) return IMPOP_OK;
    REQUIRE(m->d_vsb, "map_windows_index: the matrix has no scan index");
    REQUIRE((2 * n + 255) / 256 < 0x7FFFFFFFull, "map_windows_index: too many windows");
    ClassRanks rk;
    for (int k = KEPT; k <= top; ++k) rk.k[k] = m->idx[k];
    Carve L;
    const size_t o_in = L.take<impop_window>(n), o_out = L.take<LayoutWindow>(n);
    void *d = nullptr;
    const int rc = ctx_aux(ctx, 0, L.total(), &d);  // as map_windows_device: idle outside the all-pairs path
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(L.at<impop_window>(d, o_in), windows, n * sizeof(impop_window), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(map_edges_index_kernel, dim3((uint32_t)((2 * n + 255) / 256)), dim3(256), 0, ctx->stream, rk,
                       (const impop_window *)L.at<impop_window>(d, o_in), n, L.at<LayoutWindow>(d, o_out));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out.data(), L.at<LayoutWindow>(d, o_out), n * sizeof(LayoutWindow), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return IMPOP_OK;
}

// the distinct-row stream goes (or never came): what it allocated is freed, uskip says why
static void uniq_drop(impop_matrix *m, std::string why) {
    if (m->uidx.mask) hipFree((void *)m->uidx.mask);
    if (m->d_vuniq) hipFree(m->d_vuniq);
    if (m->d_vuniq_wt) hipFree(m->d_vuniq_wt);
    m->uidx = BlockRank();
    m->d_vuniq = nullptr;
    m->d_vuniq_wt = nullptr;
    m->n_vuniq = m->vuniq_bytes = 0;
    m->uskip = std::move(why);
}

// Drops the index from class k upward: the class's rank table and what was built on it; the classes above it lose theirs for
// want of the one below.
static void index_drop(impop_matrix *m, SiteClass k, std::string why) {
    std::string *const skip[N_CLASS] = {&m->vskip, &m->rskip, &m->sskip};
    static const char *const no_lower[N_CLASS] = {"", "no scan index", "no rare/common split"};
    for (int c = k; c < N_CLASS; ++c) {
        if (m->idx[c].mask) hipFree((void *)m->idx[c].mask);
        m->idx[c] = BlockRank();
        *skip[c] = no_lower[c];
    }
    *skip[k] = std::move(why);
    if (k <= COMMON) uniq_drop(m, k == KEPT ? "no scan index" : "no rare/common split");  // built on the common rows
    switch (k) {
    case KEPT:
        if (m->d_vsb) hipFree(m->d_vsb);
        m->d_vsb = nullptr;
        m->vg = SbGeom();
        m->vsb_bytes = m->vidx_bytes = 0;
        m->n_vkept = 0;
        [[fallthrough]];
    case COMMON:
        if (m->d_vrare) hipFree(m->d_vrare);
        m->d_vrare = nullptr;
        m->n_vrare = 0;
        [[fallthrough]];
    default:
        if (m->d_vsingle) hipFree(m->d_vsingle);
        if (m->d_vmulti) hipFree(m->d_vmulti);
        m->d_vsingle = nullptr;
        m->d_vmulti = nullptr;
        m->n_vsingle = m->vsingle_bytes = 0;
    }
}

// An allocation of the index that fails leaves the matrix without class k and the classes above it: the error is cleared, the
// matrix is still made.
static bool index_alloc(impop_matrix *m, SiteClass k, void **p, size_t bytes, const char *what) {
    if (hipMalloc(p, bytes) == hipSuccess) return true;
    (void)hipGetLastError();
    *p = nullptr;
    index_drop(m, k, std::string("hipMalloc of the ") + what + " failed");
    return false;
}

// d_tmp: per class its ne counts | per class its chunk sums | the totals
struct IndexTmp {
    size_t o_cnt[N_CLASS], o_chunk, o_total, bytes;
    IndexTmp(uint64_t ne, uint64_t n_chunks) {
        Carve L;
        for (size_t &o : o_cnt) o = L.take<uint32_t>(ne);
        o_chunk = L.take<uint64_t>(N_CLASS * n_chunks);
        o_total = L.take<uint64_t>(N_CLASS);
        bytes = L.total();
    }
};

static int index_begin(impop_ctx *ctx, impop_matrix *m, uint32_t keep_flags, IndexBuild &ib) {
    const SbGeom &g = m->g;
    ib.keep_flags = keep_flags;
    // why a class is not wanted (null: it is), and what to call its allocation.  The rare/common split: an entry (8 B) must be
    // narrower than a row, and its haplotype indices fit 16 bits; the singleton stream: read by the fixed-WPS scan kernel alone
    const struct {
        const char *skip, *what;
    } rule[N_CLASS] = {
        {keep_flags & IMPOP_KEEP_DENSE_SCAN ? "opted out (IMPOP_KEEP_DENSE_SCAN)" : nullptr, "index mask"},
        {keep_flags & IMPOP_KEEP_NO_RARE_SPLIT ? "opted out (IMPOP_KEEP_NO_RARE_SPLIT)"
         : g.wps <= 2                          ? "n_hap <= 64: a row is no wider than an 8-byte rare entry"
         : g.n_hap > 65535                     ? "n_hap > 65535: haplotype indices do not fit 16 bits"
                                               : nullptr,
         "common-site mask"},
        {keep_flags & IMPOP_KEEP_NO_SINGLE_STREAM ? "opted out (IMPOP_KEEP_NO_SINGLE_STREAM)"
         : g.wps > 16                             ? "n_hap > 512: scans run the any-n kernel, which reads the 8-byte entries"
                                                  : nullptr,
         "singleton-site mask"},
    };
    const uint64_t ne = g.n_block + 1;  // one entry past the last block: an edge at n_site maps there when 64 | n_site
    ib.n_chunks = (ne + SCAN_CHUNK - 1) / SCAN_CHUNK;
    const IndexTmp lay(ne, ib.n_chunks);
    for (int k = KEPT; k < N_CLASS; ++k) {
        void *p = nullptr;
        if (rule[k].skip) {
            index_drop(m, (SiteClass)k, rule[k].skip);
            break;
        }
        if (k == KEPT && !index_alloc(m, KEPT, &ib.d_tmp, lay.bytes, "index counts")) break;
        if (!index_alloc(m, (SiteClass)k, &p, 2 * ne * 8, rule[k].what)) break;
        m->idx[k] = {reinterpret_cast<uint64_t *>(p), reinterpret_cast<uint64_t *>(p) + ne};
        ib.out.mask[k] = reinterpret_cast<uint64_t *>(p);
        ib.out.cnt[k] = Carve::at<uint32_t>(ib.d_tmp, lay.o_cnt[k]);
        ib.n_class = k + 1;
        HIP_TRY(hipMemsetAsync(ib.out.mask[k] + g.n_block, 0, 8, ctx->stream));  // the entry past the last block holds nothing
        HIP_TRY(hipMemsetAsync(ib.out.cnt[k] + g.n_block, 0, 4, ctx->stream));
    }
    return IMPOP_OK;
}

// exclusive prefixes over ne per-block counts for n_class classes at once (chunk_sum_kernel): the totals go to d_total[k]
static void block_prefix(impop_ctx *ctx, uint32_t n_class, const PrefixArgs &a, uint64_t ne, uint64_t n_chunks, uint64_t *d_chunk,
                         uint64_t *d_total) {
    hipLaunchKernelGGL(chunk_sum_kernel, dim3((uint32_t)n_chunks, n_class), dim3(256), 0, ctx->stream, a, ne, d_chunk);
    hipLaunchKernelGGL(chunk_scan_kernel, dim3(n_class), dim3(64), 0, ctx->stream, d_chunk, n_chunks, d_total);
    hipLaunchKernelGGL(block_base_kernel, dim3((uint32_t)n_chunks, n_class), dim3(64), 0, ctx->stream, a, ne, (const uint64_t *)d_chunk);
}

// ---- distinct-row stream (internal.h, d_vuniq) ----------------------------------------------------
// One wave per 64-row block of an SB64 layout of <= 16 dwords per row, lane l holding row l.  The row is canonicalised — complemented
// within the n_hap real haplotype bits when haplotype 0 carries 1; padding bits stay 0 — and compared with every row of the block
// (64 broadcasts of a row): same = the live lanes of the block whose canonical row is this lane's.  Lanes that are not live (past
// the last row of the final block) are in no class.  w: the row as stored.
constexpr int UNIQ_WPS_MAX = 16;
__device__ inline uint64_t uniq_block_classes(const uint32_t *__restrict__ blk, uint32_t wps, uint32_t G, uint32_t r, uint32_t n_hap,
                                              bool live, uint32_t lane, uint32_t (&w)[UNIQ_WPS_MAX]) {
    uint32_t cw[UNIQ_WPS_MAX];
#pragma unroll
    for (int k = 0; k < UNIQ_WPS_MAX; ++k) w[k] = (uint32_t)k < wps ? blk[sb_index(wps, G, r, 0, lane, (uint32_t)k)] : 0u;
    const bool flip = (w[0] & 1u) != 0;
#pragma unroll
    for (int k = 0; k < UNIQ_WPS_MAX; ++k) {
        const uint32_t real = 32u * k + 32u <= n_hap ? 0xFFFFFFFFu : 32u * k < n_hap ? (1u << (n_hap - 32u * k)) - 1u : 0u;
        cw[k] = flip ? w[k] ^ real : w[k];
    }
    uint64_t same = 0;
    for (int j = 0; j < 64; ++j) {
        uint32_t diff = __shfl((int)live, j, 64) ? 0u : 1u;  // every lane takes every broadcast: no lane-dependent branch around one
#pragma unroll
        for (int k = 0; k < UNIQ_WPS_MAX; ++k) diff |= (uint32_t)__shfl((int)cw[k], j, 64) ^ cw[k];
        same |= (uint64_t)(diff == 0u) << j;
    }
    return live ? same : 0ull;
}
// a lane is its class's representative when no lower lane is in the class
__device__ inline bool uniq_is_rep(uint64_t same, uint32_t lane) { return same != 0 && (same & ((1ull << lane) - 1ull)) == 0; }

__global__ __launch_bounds__(256) void uniq_mask_kernel(const uint32_t *__restrict__ sb, uint32_t wps, uint32_t G, uint32_t r,
                                                        uint32_t n_hap, uint64_t n_row, uint64_t n_block, uint64_t *__restrict__ mask,
                                                        uint32_t *__restrict__ cnt) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t b = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= n_block) return;  // wave-uniform
    uint32_t w[UNIQ_WPS_MAX];
    const uint64_t same = uniq_block_classes(sb + b * 64ull * wps, wps, G, r, n_hap, b * 64 + lane < n_row, lane, w);
    const uint64_t reps = __ballot(uniq_is_rep(same, lane));
    if (lane == 0) { mask[b] = reps; cnt[b] = (uint32_t)__popcll(reps); }
}
// the representatives' rows, as stored, to their places in the stream (base: the representatives before each block), and their weights
__global__ __launch_bounds__(256) void uniq_gather_kernel(const uint32_t *__restrict__ sb, uint32_t wps, uint32_t G, uint32_t r,
                                                          uint32_t n_hap, uint64_t n_row, uint64_t n_block,
                                                          const uint64_t *__restrict__ base, uint64_t n_uniq, uint32_t *__restrict__ out,
                                                          uint8_t *__restrict__ out_wt) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t b = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= n_block) return;  // wave-uniform
    uint32_t w[UNIQ_WPS_MAX];
    const uint64_t same = uniq_block_classes(sb + b * 64ull * wps, wps, G, r, n_hap, b * 64 + lane < n_row, lane, w);
    const bool rep = uniq_is_rep(same, lane);
    const uint64_t reps = __ballot(rep);
    if (!rep) return;
    const uint64_t dest = base[b] + (uint64_t)__popcll(reps & ((1ull << lane) - 1ull));
    if (dest >= n_uniq) return;  // cannot happen: base is the prefix of these very counts
#pragma unroll
    for (int k = 0; k < UNIQ_WPS_MAX; ++k)
        if ((uint32_t)k < wps) out[sb_index(wps, G, r, dest >> 6, (uint32_t)(dest & 63), (uint32_t)k)] = w[k];
    out_wt[dest] = (uint8_t)__popcll(same);  // 1..64
}

// the stream is kept when its representatives are at most IMPOP_UNIQ_MAX_NUM / IMPOP_UNIQ_MAX_DEN of the common rows
constexpr uint64_t IMPOP_UNIQ_MAX_NUM = 3, IMPOP_UNIQ_MAX_DEN = 4;

// Builds the distinct-row stream on top of a finished split index (d_vsb holds the common rows), or records why there is none.
// Like the rest of the index it never fails the matrix: an allocation that cannot be had leaves the matrix without the stream.
static int unique_rows_build(impop_ctx *ctx, impop_matrix *m, uint32_t keep_flags) {
    static const bool env_off = env_is("IMPOP_NO_UNIQUE_ROWS", '1');
    const SbGeom &g = m->g;
    const uint64_t n_row = m->vg.n_site, nvb = m->vg.n_block, ne = nvb + 1, n_chunks = (ne + SCAN_CHUNK - 1) / SCAN_CHUNK;
    const char *skip = keep_flags & IMPOP_KEEP_NO_UNIQUE_ROWS ? "opted out (IMPOP_KEEP_NO_UNIQUE_ROWS)"
                       : env_off                               ? "opted out (IMPOP_NO_UNIQUE_ROWS=1)"
                       : !m->d_vrare                           ? "no rare/common split"
                       : g.wps > UNIQ_WPS_MAX                  ? "n_hap > 512: scans run the any-n kernel, which reads the rows"
                       : n_row == 0                            ? "no common rows"
                                                               : nullptr;
    if (skip) {
        uniq_drop(m, skip);
        return IMPOP_OK;
    }
    REQUIRE((nvb + 3) / 4 < 0x7FFFFFFFull && n_chunks < 0x7FFFFFFFull, "distinct-row stream: too many common rows for one launch");
    Carve L;
    const size_t o_cnt = L.take<uint32_t>(ne), o_chunk = L.take<uint64_t>(n_chunks), o_total = L.take<uint64_t>(1);
    struct Owned {  // freed on every way out unless handed on
        void *p = nullptr;
        ~Owned() { if (p) hipFree(p); }
    } tmp, rank, rows, wts;
    auto none = [&](std::string why) {
        (void)hipGetLastError();
        uniq_drop(m, std::move(why));
        return IMPOP_OK;
    };
    if (hipMalloc(&tmp.p, L.total()) != hipSuccess) { tmp.p = nullptr; return none("hipMalloc of the distinct-row counts failed"); }
    if (hipMalloc(&rank.p, 2 * ne * 8) != hipSuccess) { rank.p = nullptr; return none("hipMalloc of the distinct-row mask failed"); }
    uint64_t *mask = reinterpret_cast<uint64_t *>(rank.p), *base = mask + ne, *d_total = L.at<uint64_t>(tmp.p, o_total);
    uint32_t *cnt = L.at<uint32_t>(tmp.p, o_cnt);
    HIP_TRY(hipMemsetAsync(mask + nvb, 0, 8, ctx->stream));  // the entry past the last block holds nothing
    HIP_TRY(hipMemsetAsync(cnt + nvb, 0, 4, ctx->stream));
    hipLaunchKernelGGL(uniq_mask_kernel, dim3((uint32_t)((nvb + 3) / 4)), dim3(256), 0, ctx->stream, (const uint32_t *)m->d_vsb, g.wps, g.G,
                       g.r, g.n_hap, n_row, nvb, mask, cnt);
    block_prefix(ctx, 1, PrefixArgs{{cnt}, {base}}, ne, n_chunks, L.at<uint64_t>(tmp.p, o_chunk), d_total);
    HIP_TRY(hipGetLastError());
    uint64_t n_uniq = 0;
    HIP_TRY(hipMemcpyAsync(&n_uniq, d_total, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (n_uniq * IMPOP_UNIQ_MAX_DEN > n_row * IMPOP_UNIQ_MAX_NUM) {
        char why[160];
        snprintf(why, sizeof why, "%llu distinct of %llu common rows: above %llu/%llu", (unsigned long long)n_uniq, (unsigned long long)n_row,
                 (unsigned long long)IMPOP_UNIQ_MAX_NUM, (unsigned long long)IMPOP_UNIQ_MAX_DEN);
        return none(why);
    }
    // rows: whole blocks and, as for d_vsb, one block of slack; weights: whole blocks and 64 bytes of slack.  All zero first: the
    // rows past the last representative add nothing to any sum whatever their weight
    const uint64_t nub = (n_uniq + 63) / 64, row_bytes = (nub + 1) * 64ull * g.wps * 4ull + 256, wt_bytes = nub * 64 + 64;
    if (hipMalloc(&rows.p, row_bytes) != hipSuccess) { rows.p = nullptr; return none("hipMalloc of the distinct rows failed"); }
    if (hipMalloc(&wts.p, wt_bytes) != hipSuccess) { wts.p = nullptr; return none("hipMalloc of the distinct rows' weights failed"); }
    m->uidx = {mask, base};
    m->d_vuniq = reinterpret_cast<uint32_t *>(rows.p);
    m->d_vuniq_wt = reinterpret_cast<uint8_t *>(wts.p);
    rank.p = rows.p = wts.p = nullptr;  // the matrix's from here (uniq_drop frees them)
    m->n_vuniq = n_uniq;
    m->vuniq_bytes = 2 * ne * 8 + row_bytes + wt_bytes;
    m->uskip.clear();
    HIP_TRY(hipMemsetAsync(m->d_vuniq, 0, row_bytes, ctx->stream));
    HIP_TRY(hipMemsetAsync(m->d_vuniq_wt, 0, wt_bytes, ctx->stream));
    hipLaunchKernelGGL(uniq_gather_kernel, dim3((uint32_t)((nvb + 3) / 4)), dim3(256), 0, ctx->stream, (const uint32_t *)m->d_vsb, g.wps,
                       g.G, g.r, g.n_hap, n_row, nvb, (const uint64_t *)base, n_uniq, m->d_vuniq, m->d_vuniq_wt);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // the counts go
    m->vidx_bytes += m->vuniq_bytes;
    return IMPOP_OK;
}

static int index_finish(impop_ctx *ctx, impop_matrix *m, IndexBuild &ib) {
    if (!ib.n_class) return IMPOP_OK;
    const SbGeom &g = m->g;
    const uint64_t nb = g.n_block, ne = nb + 1;
    const IndexTmp lay(ne, ib.n_chunks);
    uint64_t *d_total = Carve::at<uint64_t>(ib.d_tmp, lay.o_total);
    REQUIRE(ib.n_chunks < 0x7FFFFFFFull && (nb + 255) / 256 < 0x7FFFFFFFull, "scan index: matrix too long for one launch");
    PrefixArgs pa{};
    for (uint32_t k = 0; k < ib.n_class; ++k) {
        pa.cnt[k] = ib.out.cnt[k];
        pa.base[k] = ib.out.mask[k] + ne;
    }
    block_prefix(ctx, ib.n_class, pa, ne, ib.n_chunks, Carve::at<uint64_t>(ib.d_tmp, lay.o_chunk), d_total);
    HIP_TRY(hipGetLastError());
    uint64_t totals[N_CLASS] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(totals, d_total, ib.n_class * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const uint64_t n_kept = totals[KEPT];
    if (n_kept * IMPOP_INDEX_MAX_KEPT_INV > g.n_site) {
        char why[160];
        snprintf(why, sizeof why, "%llu of %llu sites vary: above 1/%llu", (unsigned long long)n_kept, (unsigned long long)g.n_site,
                 (unsigned long long)IMPOP_INDEX_MAX_KEPT_INV);
        index_drop(m, KEPT, why);
        return IMPOP_OK;
    }
    // the rare entries first: when they cannot be had, d_vsb holds every kept site (the unsplit index)
    if (ib.n_class > COMMON) {
        m->n_vrare = n_kept - totals[COMMON];
        if (index_alloc(m, COMMON, (void **)&m->d_vrare, std::max<uint64_t>(m->n_vrare, 1) * 8, "rare entries")) m->rskip.clear();
    }
    // ... and their two packed streams; without them the split index is what it was
    uint64_t single_pad = 0;  // bytes of d_vsingle: whole 8-byte words, then 8 bytes of slack
    if (ib.n_class > SINGLE && m->d_vrare) {
        m->n_vsingle = totals[SINGLE];
        single_pad = (m->n_vsingle * 2 + 7) / 8 * 8 + 8;
        void *sg = nullptr, *mu = nullptr;
        if (hipMalloc(&sg, single_pad) != hipSuccess || hipMalloc(&mu, std::max<uint64_t>(m->n_vrare - m->n_vsingle, 1) * 8) != hipSuccess) {
            (void)hipGetLastError();
            if (sg) hipFree(sg);
            index_drop(m, SINGLE, "hipMalloc of the singleton stream failed");
        } else {
            m->d_vsingle = reinterpret_cast<uint16_t *>(sg);
            m->d_vmulti = reinterpret_cast<uint64_t *>(mu);
            m->vsingle_bytes = 2 * ne * 8 + single_pad + std::max<uint64_t>(m->n_vrare - m->n_vsingle, 1) * 8;
            m->sskip.clear();
            HIP_TRY(hipMemsetAsync((char *)sg + m->n_vsingle * 2, 0xFF, single_pad - m->n_vsingle * 2, ctx->stream));
        }
    }
    const bool split = m->d_vrare != nullptr;
    const BlockRank &stream = m->idx[split ? COMMON : KEPT];      // the class of the SB64 copy
    const uint64_t n_stream = split ? totals[COMMON] : n_kept;  // ... and its sites
    m->n_vkept = n_kept;
    m->vg = make_geom(g.n_hap, n_stream);
    m->vsb_bytes = m->vg.n_block * 64ull * g.wps * 4ull;
    const uint64_t slack = 64ull * g.wps * 4ull + 256;  // as alloc_matrix: one block past the end may be prefetched
    void *vsb = nullptr;
    if (!index_alloc(m, KEPT, &vsb, m->vsb_bytes + slack, "kept-site layout")) return IMPOP_OK;
    m->d_vsb = reinterpret_cast<uint32_t *>(vsb);
    HIP_TRY(hipMemsetAsync((char *)vsb + m->vsb_bytes, 0, slack, ctx->stream));
    if (n_stream) {
        if (!index_alloc(m, KEPT, (void **)&ib.d_pos, n_stream * 8, "kept-site positions")) return IMPOP_OK;
        REQUIRE((m->vg.n_block + 3) / 4 < 0x7FFFFFFFull, "scan index: too many kept sites for one launch");
        hipLaunchKernelGGL(kept_pos_kernel, dim3((uint32_t)((nb + 255) / 256)), dim3(256), 0, ctx->stream, stream.mask, stream.base, nb, ib.d_pos);
        hipLaunchKernelGGL(gather_kept_kernel, dim3((uint32_t)((m->vg.n_block + 3) / 4)), dim3(256), 0, ctx->stream, m->d_sb, g.wps,
                           g.G, g.r, ib.d_pos, n_stream, m->vg.n_block, m->d_vsb);
        HIP_TRY(hipGetLastError());
    }
    if (split && m->n_vrare) {
        ClassRanks rk;
        for (int k = KEPT; k <= (m->d_vsingle ? SINGLE : COMMON); ++k) rk.k[k] = m->idx[k];
        hipLaunchKernelGGL(rare_entries_kernel, dim3((uint32_t)((nb + 255) / 256)), dim3(256), 0, ctx->stream, m->d_sb, g.wps, g.G, g.r,
                           g.n_hap, rk, nb, m->d_vrare, m->d_vsingle, m->d_vmulti);
        HIP_TRY(hipGetLastError());
    }
    m->vidx_bytes = 2 * ne * 8 + m->vsb_bytes + slack + (split ? 2 * ne * 8 + std::max<uint64_t>(m->n_vrare, 1) * 8 : 0) + m->vsingle_bytes;
    m->vskip.clear();
    return unique_rows_build(ctx, m, ib.keep_flags);
}

}  // namespace impop

IMPOP_API int impop_matrix_compact(impop_ctx *ctx, const impop_matrix *in, impop_matrix **out) {
    REQUIRE(ctx && in && out, "impop_matrix_compact: NULL argument");
    *out = nullptr;
    REQUIRE(!in->compact, "impop_matrix_compact: matrix is already compacted");
    HIP_TRY(hipSetDevice(ctx->device));
    const SbGeom &g = in->g;
    const uint64_t nb = g.n_block, n_chunks = (nb + SCAN_CHUNK - 1) / SCAN_CHUNK;
    REQUIRE((nb + 3) / 4 < 0x7FFFFFFFull, "impop_matrix_compact: matrix too long for one launch");
    Carve L;
    const size_t o_mask = L.take<uint64_t>(nb), o_cnt = L.take<uint32_t>(nb), o_base = L.take<uint64_t>(nb), o_chunk = L.take<uint64_t>(n_chunks),
                 o_total = L.take<uint64_t>(1);
    ClassOut kept;
    void *d = nullptr;
    int rc = ctx_scratch(ctx, L.total(), &d);
    if (rc) return rc;
    uint64_t *d_mask = L.at<uint64_t>(d, o_mask), *d_base = L.at<uint64_t>(d, o_base), *d_chunk = L.at<uint64_t>(d, o_chunk),
             *d_total = L.at<uint64_t>(d, o_total);
    kept.mask[KEPT] = d_mask;
    kept.cnt[KEPT] = L.at<uint32_t>(d, o_cnt);
    uint64_t n_kept = 0;
    // a source that kept its hap-major copy hands the all-pairs path on: the compacted matrix gets its own RB32
    // operand; the bitmap of the dropped all-ones sites is built for every compacted matrix (their count — for a weighted
    // source the sum of their weights, from host prefix sums built below — comes back as a per-window constant of the
    // all-pairs path; impop_diploid_scan adds it to every individual's hom_alt)
    const bool want_pairs = in->d_rb != nullptr;
    uint64_t *d_ones = nullptr;
    if (nb) HIP_TRY(hipMalloc((void **)&d_ones, nb * 8 + 256));
    if (nb) {
        const uint32_t wide_grid = (uint32_t)std::min<uint64_t>((nb + 3) / 4, 32ull * (uint64_t)(ctx->n_cu > 0 ? ctx->n_cu : 256));
        hipLaunchKernelGGL(variable_mask_kernel, dim3(wide_grid), dim3(256), 0, ctx->stream, in->d_sb, g.wps, g.G, g.r, nb, g.n_site,
                           g.n_hap, kept, d_ones);
        block_prefix(ctx, 1, PrefixArgs{{kept.cnt[KEPT]}, {d_base}}, nb, n_chunks, d_chunk, d_total);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&n_kept, d_total, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    impop_matrix *m = nullptr;
    rc = alloc_matrix(ctx, g.n_hap, n_kept, want_pairs, &m);
    if (rc) {
        if (d_ones) hipFree(d_ones);
        return rc;
    }
    m->d_onesmap = reinterpret_cast<uint32_t *>(d_ones);  // uint64 per 64-site block == two dwords of 32 sites
    auto fail = [&](int code) {
        impop_matrix_free(ctx, m);
        return code;
    };
    m->compact = true;
    m->vskip = "compacted matrix (every site is kept)";
    m->rskip = "no scan index";
    m->sskip = "no rare/common split";
    m->n_site_orig = g.n_site;
    m->pos.resize(n_kept);
    if (n_kept) {
        uint64_t *d_pos = nullptr;
        hipError_t e = hipMalloc((void **)&d_pos, n_kept * 8);
        if (e != hipSuccess) return fail(hip_fail(e, "hipMalloc(positions)", __FILE__, __LINE__));
        auto fail2 = [&](hipError_t err, const char *what) {
            hipFree(d_pos);
            return fail(hip_fail(err, what, __FILE__, __LINE__));
        };
        if ((e = hipMemsetAsync(m->d_sb, 0, m->sb_bytes, ctx->stream)) != hipSuccess) return fail2(e, "hipMemsetAsync");
        const uint32_t wide_grid = (uint32_t)std::min<uint64_t>((nb + 3) / 4, 32ull * (uint64_t)(ctx->n_cu > 0 ? ctx->n_cu : 256));
        hipLaunchKernelGGL(gather_variable_kernel, dim3(wide_grid), dim3(256), 0, ctx->stream, in->d_sb, g.wps, g.G, g.r, nb, d_mask,
                           d_base, m->d_sb, d_pos);
        if ((e = hipGetLastError()) != hipSuccess) return fail2(e, "gather_variable_kernel");
        if ((e = hipMemcpyAsync(m->pos.data(), d_pos, n_kept * 8, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess)
            return fail2(e, "hipMemcpyAsync(positions)");
        if (want_pairs) {
            const int rc2 = launch_sb_to_hm(ctx, m->d_sb, m->g, 0, m->g.n_block, m->d_rb, 0, m->n_hap_pad, m->rb_nb, m->phi_row);
            if (rc2) { hipFree(d_pos); return fail(rc2); }
        }
        if ((e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return fail2(e, "hipStreamSynchronize");
        m->d_pos = d_pos;  // kept: window edges are mapped on the device (map_windows_device)
    }
    m->pos_coarse.clear();
    for (size_t k = 0; k < m->pos.size(); k += (size_t)1 << POS_COARSE_SHIFT) m->pos_coarse.push_back(m->pos[k]);
    if (!in->wt_prefix.empty()) {
        // weighted input: the kept columns keep their weights; a window's W is still the sum over ALL its original
        // columns (monomorphic ones included), so the prefix sums of the original weights travel along
        m->wt_prefix = in->wt_prefix;
        if (n_kept) {
            std::vector<uint32_t> kept(n_kept);
            for (uint64_t k = 0; k < n_kept; ++k) kept[k] = (uint32_t)(in->wt_prefix[m->pos[k] + 1] - in->wt_prefix[m->pos[k]]);
            hipError_t e;
            if ((e = hipMalloc((void **)&m->d_wt, n_kept * 4ull)) != hipSuccess) return fail(hip_fail(e, "hipMalloc(weights)", __FILE__, __LINE__));
            if ((e = hipMemcpy(m->d_wt, kept.data(), n_kept * 4ull, hipMemcpyHostToDevice)) != hipSuccess)
                return fail(hip_fail(e, "hipMemcpy(weights)", __FILE__, __LINE__));
            if (want_pairs) {
                m->kept_wt_prefix.resize(n_kept + 1);
                m->kept_wt_prefix[0] = 0;
                for (uint64_t k = 0; k < n_kept; ++k) m->kept_wt_prefix[k + 1] = m->kept_wt_prefix[k] + kept[k];
            }
        }
        if (want_pairs && m->kept_wt_prefix.empty()) m->kept_wt_prefix.assign(1, 0);  // nothing kept
        if (want_pairs) {  // weights of the dropped all-ones sites, as prefix sums over the original coordinates
            std::vector<uint64_t> ones(nb);
            hipError_t e;
            if (nb && (e = hipMemcpy(ones.data(), d_ones, nb * 8, hipMemcpyDeviceToHost)) != hipSuccess)
                return fail(hip_fail(e, "hipMemcpy(all-ones bitmap)", __FILE__, __LINE__));
            m->ones_wt_prefix.resize(g.n_site + 1);
            uint64_t acc = 0;
            for (uint64_t i = 0; i < g.n_site; ++i) {
                m->ones_wt_prefix[i] = acc;
                if ((ones[i >> 6] >> (i & 63)) & 1ull) acc += in->wt_prefix[i + 1] - in->wt_prefix[i];
            }
            m->ones_wt_prefix[g.n_site] = acc;
        }
    }
    *out = m;
    return IMPOP_OK;
}

namespace impop {
void matrix_drop_derived(const impop_matrix *m) {
    if (m->d_wplanes) hipFree(m->d_wplanes);
    if (m->d_rb_masked) hipFree(m->d_rb_masked);
    if (m->d_segmap) hipFree(m->d_segmap);
    m->d_wplanes = nullptr; m->d_rb_masked = nullptr; m->d_segmap = nullptr;
    m->wplane_bits = 0; m->wplane_stride = 0;
}
}  // namespace impop

IMPOP_API int impop_matrix_set_site_weights(impop_ctx *ctx, impop_matrix *m, const uint32_t *weights_host) {
    REQUIRE(ctx && m, "impop_matrix_set_site_weights: NULL argument");
    NOT_COMPACT(m, "impop_matrix_set_site_weights");
    REQUIRE(m->users == 0, "impop_matrix_set_site_weights: %d scan plan(s) were built with the current weights; destroy them first",
            m->users);
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // launches in flight may still read the old weights
    if (m->d_wt) {
        HIP_TRY(hipFree(m->d_wt));
        m->d_wt = nullptr;
    }
    matrix_drop_derived(m);  // weight planes / masked operand belong to the old weights
    m->wt_prefix.clear();
    if (!weights_host) return IMPOP_OK;
    // host prefix sums: a window's W = sum of its columns' weights, looked up when a plan is built
    m->wt_prefix.resize(m->g.n_site + 1);
    m->wt_prefix[0] = 0;
    for (uint64_t i = 0; i < m->g.n_site; ++i) m->wt_prefix[i + 1] = m->wt_prefix[i] + weights_host[i];
    if (m->g.n_site == 0) return IMPOP_OK;
    HIP_TRY(hipMalloc((void **)&m->d_wt, m->g.n_site * 4ull));
    HIP_TRY(hipMemcpy(m->d_wt, weights_host, m->g.n_site * 4ull, hipMemcpyHostToDevice));
    return IMPOP_OK;
}

IMPOP_API int impop_matrix_positions(const impop_matrix *m, uint64_t first, uint64_t count, uint64_t *out, uint64_t *n_site_orig) {
    REQUIRE(m, "impop_matrix_positions: matrix is NULL");
    REQUIRE(m->compact, "impop_matrix_positions: not a compacted matrix");
    REQUIRE(first <= m->pos.size() && count <= m->pos.size() - first, "impop_matrix_positions: range out of bounds");
    REQUIRE(count == 0 || out, "impop_matrix_positions: out is NULL");
    for (uint64_t i = 0; i < count; ++i) out[i] = m->pos[first + i];
    if (n_site_orig) *n_site_orig = m->n_site_orig;
    return IMPOP_OK;
}

IMPOP_API int impop_matrix_info(const impop_matrix *m, uint32_t *n_hap, uint64_t *n_site, uint64_t *device_bytes,
                                uint32_t *bytes_per_site) {
    REQUIRE(m, "impop_matrix_info: matrix is NULL");
    if (n_hap) *n_hap = m->g.n_hap;
    if (n_site) *n_site = m->g.n_site;
    if (device_bytes) *device_bytes = m->sb_bytes + m->rb_bytes;
    if (bytes_per_site) *bytes_per_site = m->g.wps * 4;
    return IMPOP_OK;
}

IMPOP_API int impop_matrix_scan_index_info(const impop_matrix *m, uint64_t *n_kept, uint64_t *index_bytes, char *why, size_t why_len) {
    REQUIRE(m, "impop_matrix_scan_index_info: matrix is NULL");
    if (n_kept) *n_kept = m->d_vsb ? m->n_vkept : 0;
    if (index_bytes) *index_bytes = m->d_vsb ? m->vidx_bytes : 0;
    if (why && why_len) snprintf(why, why_len, "%s", m->d_vsb ? "" : m->vskip.c_str());
    return IMPOP_OK;
}

IMPOP_API int impop_matrix_scan_split_info(const impop_matrix *m, uint64_t *n_rare, uint64_t *n_common, uint64_t *rare_bytes,
                                           char *why, size_t why_len) {
    REQUIRE(m, "impop_matrix_scan_split_info: matrix is NULL");
    const bool split = m->d_vsb && m->d_vrare;
    if (n_rare) *n_rare = split ? m->n_vrare : 0;
    if (n_common) *n_common = split ? m->vg.n_site : 0;
    if (rare_bytes) *rare_bytes = split ? m->n_vrare * 8 : 0;
    if (why && why_len) snprintf(why, why_len, "%s", split ? "" : m->rskip.c_str());
    return IMPOP_OK;
}

IMPOP_API int impop_matrix_scan_single_info(const impop_matrix *m, uint64_t *n_single, uint64_t *n_multi, uint64_t *stream_bytes,
                                            char *why, size_t why_len) {
    REQUIRE(m, "impop_matrix_scan_single_info: matrix is NULL");
    const bool built = m->d_vsb && m->d_vrare && m->d_vsingle;
    const bool has = built && m->wt_prefix.empty();  // no scan of a weighted matrix reads the index
    if (n_single) *n_single = has ? m->n_vsingle : 0;
    if (n_multi) *n_multi = has ? m->n_vrare - m->n_vsingle : 0;
    if (stream_bytes) *stream_bytes = has ? m->vsingle_bytes : 0;
    if (why && why_len) snprintf(why, why_len, "%s", has ? "" : built ? "site weights: scans stream the dense layout" : m->sskip.c_str());
    return IMPOP_OK;
}

IMPOP_API int impop_matrix_scan_unique_info(const impop_matrix *m, uint64_t *n_unique, uint64_t *n_common, uint64_t *stream_bytes,
                                            char *why, size_t why_len) {
    REQUIRE(m, "impop_matrix_scan_unique_info: matrix is NULL");
    const bool built = m->d_vsb && m->d_vrare && m->d_vuniq;
    const bool has = built && m->wt_prefix.empty();  // no scan of a weighted matrix reads the index
    if (n_unique) *n_unique = has ? m->n_vuniq : 0;
    if (n_common) *n_common = has ? m->vg.n_site : 0;
    if (stream_bytes) *stream_bytes = has ? m->vuniq_bytes : 0;
    if (why && why_len) snprintf(why, why_len, "%s", has ? "" : built ? "site weights: scans stream the dense layout" : m->uskip.c_str());
    return IMPOP_OK;
}

IMPOP_API int impop_matrix_free(impop_ctx *ctx, impop_matrix *m) {
    if (!m) return IMPOP_OK;
    REQUIRE(m->users == 0, "impop_matrix_free: %d scan plan(s) still reference this matrix; destroy them first", m->users);
    if (ctx) {
        hipSetDevice(ctx->device);
        hipStreamSynchronize(ctx->stream);
    }
    if (m->d_sb) hipFree(m->d_sb);
    if (m->d_rb) hipFree(m->d_rb);
    if (m->d_wt) hipFree(m->d_wt);
    if (m->d_onesmap) hipFree(m->d_onesmap);
    if (m->d_pos) hipFree(m->d_pos);
    index_drop(m, KEPT, "");
    matrix_drop_derived(m);
    delete m;
    return IMPOP_OK;
}
