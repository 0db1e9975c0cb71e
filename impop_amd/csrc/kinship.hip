// kinship.hip — impop_genotypes_* (the per-individual genotype planes H = h1 ^ h2, A = h1 & h2, built on the device straight into
// the Gram kernel's RB32 operand layout) and impop_kinship_scan: its kernels, its PairEpilogue (pair_front.h) and the entry point.
// Per window and pair of individuals the 3 x 3 joint genotype table from four Gram entries and the diagonals (kin_math.h).
#include "hap_words.h"
#include "kin_math.h"
#include "pair_front.h"

// the genotype planes of impop_genotypes_create: a matrix the Gram front end accepts (2N rows, RB32 operand alone), as its own type
struct impop_genotypes {
    impop_matrix *planes = nullptr;
    uint32_t n_ind = 0;
};

namespace impop {

// ---- the planes ----------------------------------------------------------------------------------------------------------------
// One wave per 64-site block of the source.  The ballot transpose (hap_words.h) turns the block's site-major dwords into one
// 64-site word per paired haplotype, parked in the wave's slice of LDS at position 2 i (h1 of individual i) or 2 i + 1 (h2).  The
// wave then writes the block's cell of every 32-row group of the operand: lane l holds dword l & 1 of row 32 g + (l >> 1), so a
// group's 32 dword pairs leave as one contiguous 256-byte store.  Rows N .. 2N - 1 are the A planes; the rows of a group past 2N
// are written as zeros, the groups past them and the slack cells stay as the allocation's memset left them.
constexpr size_t GENO_LDS_BUDGET = 64 * 1024;

__global__ __launch_bounds__(256) void geno_planes_kernel(const uint32_t *__restrict__ sb, uint32_t wps, uint32_t G, uint32_t r,
                                                          uint64_t n_block, uint64_t n_site, const int32_t *__restrict__ ppos,
                                                          const uint32_t *__restrict__ pmask, uint32_t N, uint32_t *__restrict__ rb,
                                                          uint64_t rb_nb) {
    extern __shared__ uint64_t geno_words[];
    const uint32_t lane = threadIdx.x & 63, wave = (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6), n_waves = blockDim.x >> 6;
    const uint64_t b = (uint64_t)blockIdx.x * n_waves + wave;
    const bool live = b < n_block;  // wave-uniform; every wave reaches the barrier
    uint64_t *w = geno_words + (size_t)wave * 2 * N;
    if (live) {
        const uint64_t left = n_site - b * 64;  // sites beyond n_site in the last block are zero
        const uint64_t edge = left < 64 ? (1ull << left) - 1ull : ~0ull;
        hap_block_words(sb + b * 64ull * wps, G, r, lane, edge, ppos, pmask, [&](uint32_t pp, uint64_t word) { w[pp] = word; });
    }
    __syncthreads();
    if (!live) return;
    const uint32_t n_group = (2 * N + 31) / 32;
    for (uint32_t g = 0; g < n_group; ++g) {
        const uint32_t row = 32 * g + (lane >> 1);
        uint64_t v = 0;
        if (row < N) v = w[2 * row] ^ w[2 * row + 1];
        else if (row < 2 * N) v = w[2 * (row - N)] & w[2 * (row - N) + 1];
        rb[((uint64_t)g * rb_nb + b) * 64 + lane] = (lane & 1) ? (uint32_t)(v >> 32) : (uint32_t)v;
    }
}

// rows of the operand back as row-major 64-bit words of the sites [s0, s1): one thread per (row, word)
__global__ void geno_download_kernel(const uint32_t *__restrict__ rb, uint64_t rb_nb, uint32_t n_rows, uint64_t s0, uint64_t s1,
                                     uint64_t nw, uint64_t *__restrict__ out) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (uint64_t)n_rows * nw) return;
    const uint32_t row = (uint32_t)(t / nw);
    const uint64_t s = s0 + 64 * (t % nw), cell = s >> 6;
    const uint32_t sh = (uint32_t)(s & 63);
    auto word = [&](uint64_t c) {  // c <= n_block: inside the slack cells, which are zero
        const uint32_t *p = rb + ((uint64_t)(row >> 5) * rb_nb + c) * 64 + 2 * (row & 31);
        return (uint64_t)p[0] | ((uint64_t)p[1] << 32);
    };
    uint64_t v = word(cell) >> sh;
    if (sh) v |= word(cell + 1) << (64 - sh);
    if (s1 - s < 64) v &= (1ull << (s1 - s)) - 1ull;
    out[t] = v;
}

// ---- the epilogue, on a chunk's Gram problems of the 2N plane rows [H_0 .. H_{N-1}, A_0 .. A_{N-1}] -------------------------------
struct KinshipOut {
    impop_kin_window *windows;  // n_problems
    impop_kin_watch *watch;     // n_problems x n_watch, or nullptr
    uint64_t *totals;           // N (N - 1) / 2 x 9, ADDED to (one owner per entry), or nullptr
    uint32_t *diag;             // scratch: n_problems x 2N, het then alt per problem (the windows kernel writes, the totals kernel reads)
    uint64_t *part;             // scratch: kinship_total_slices x N (N - 1) / 2 x 9 when there is more than one slice, else unused
};
constexpr uint64_t KIN_TOTALS_THREADS = 1ull << 19;  // (pair, slice) threads the totals kernel aims at
constexpr uint32_t KIN_TOTALS_MAX_SLICES = 64;

// the table of the pair i < j of problem S.  gram_at adds a compacted problem's constant (its dropped all-ones sites) to every entry:
// it belongs to alt and AA alone, so the H entries give it back
__device__ __forceinline__ bool kin_pair_table(const SimView &S, uint32_t N, uint32_t i, uint32_t j, uint32_t het_i, uint32_t alt_i,
                                               uint32_t het_j, uint32_t alt_j, KinTable &k) {
    const int64_t HH = gram_at(S, i, j) - S.add, HA = gram_at(S, i, N + j) - S.add, AH = gram_at(S, j, N + i) - S.add,
                  AA = gram_at(S, N + i, N + j);
    return kin_table((int64_t)S.W, het_i, alt_i, het_j, alt_j, HH, HA, AH, AA, k);
}

constexpr int KIN_T = 256;

// One workgroup per window.  The diagonals go to LDS (and to O.diag for the totals kernel); a wave owns a row i and its lanes the
// j > i, so HH, HA and AA are read along Gram rows and AH strided down a column, as pairdist.hip reads its lower part.
__global__ __launch_bounds__(KIN_T) void kinship_window_kernel(SimBatch batch, uint32_t N, int64_t num, int64_t den,
                                                              const uint32_t *__restrict__ watch, uint32_t n_watch, KinshipOut O,
                                                              uint32_t *__restrict__ diag_out, uint32_t *__restrict__ err) {
    __shared__ uint32_t het[IMPOP_KINSHIP_MAX_N], alt[IMPOP_KINSHIP_MAX_N];
    __shared__ uint64_t red[KIN_T / 64];
    const uint64_t w = blockIdx.x;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const SimView S = sim_view(batch, w);
    for (uint32_t i = tid; i < N; i += KIN_T) {
        const int64_t h = gram_at(S, i, i) - S.add, a = gram_at(S, N + i, N + i);
        het[i] = (uint32_t)h; alt[i] = (uint32_t)a;
        diag_out[w * 2 * N + i] = (uint32_t)h;
        diag_out[w * 2 * N + N + i] = (uint32_t)a;
    }
    __syncthreads();
    uint64_t hh = 0, i0 = 0, i2 = 0, n_rel = 0, n_und = 0;
    bool bad = false;
    for (uint32_t i = wave; i + 1 < N; i += KIN_T / 64)
        for (uint32_t j = i + 1 + lane; j < N; j += 64) {
            KinTable k;
            bad |= !kin_pair_table(S, N, i, j, het[i], alt[i], het[j], alt[j], k);
            hh += (uint64_t)kin_het_het(k); i0 += (uint64_t)kin_ibs0(k); i2 += (uint64_t)kin_ibs2(k);
            const uint32_t m = het[i] < het[j] ? het[i] : het[j];
            n_und += m == 0 ? 1u : 0u;
            n_rel += kin_related(het[i], het[j], kin_het_het(k), kin_ibs0(k), num, den) ? 1u : 0u;
        }
    for (uint32_t q = tid; q < n_watch; q += KIN_T) {
        const uint32_t a = watch[2 * q], b = watch[2 * q + 1], i = a < b ? a : b, j = a < b ? b : a;
        KinTable k;
        bad |= !kin_pair_table(S, N, i, j, het[i], alt[i], het[j], alt[j], k);
        O.watch[w * n_watch + q] = impop_kin_watch{(uint32_t)kin_het_het(k), (uint32_t)kin_ibs0(k), het[a], het[b]};
    }
    if (bad) atomicOr(err, DEV_ERR_KINSHIP);
    hh = block_sum_u64_n<KIN_T>(hh, red); i0 = block_sum_u64_n<KIN_T>(i0, red); i2 = block_sum_u64_n<KIN_T>(i2, red);
    n_rel = block_sum_u64_n<KIN_T>(n_rel, red); n_und = block_sum_u64_n<KIN_T>(n_und, red);
    if (tid == 0) {
        impop_kin_window r;
        r.n_ind = N; r.n_sites = (uint32_t)S.W; r.n_pairs = (uint64_t)N * (N - 1) / 2;
        r.het_het = hh; r.ibs0 = i0; r.ibs2 = i2; r.n_related = (uint32_t)n_rel; r.n_undefined = (uint32_t)n_und;
        O.windows[w] = r;
    }
}

// One thread per (pair, slice): row i = blockIdx.y, j along x (the same access pattern), and slice z = blockIdx.z takes the chunk's
// windows z, z + Z, ... in turn.  With one slice the thread is the one owner of its nine totals and adds to them once per chunk;
// with several it leaves its nine sums in `part` (slice-major) and kinship_totals_reduce_kernel, one thread per entry, adds the
// slices in their order: integer adds with one owner per entry either way.  (A lone thread per pair walks 4096 windows one memory
// latency at a time: 7.8 ms for 232 individuals against 1.0 ms for the window kernel.)
__global__ __launch_bounds__(KIN_T) void kinship_totals_kernel(SimBatch batch, uint64_t n_problems, uint32_t N,
                                                              const uint32_t *__restrict__ diag, uint64_t *__restrict__ totals,
                                                              uint64_t *__restrict__ part) {
    const uint32_t i = blockIdx.y, j = i + 1 + blockIdx.x * KIN_T + threadIdx.x;
    if (j >= N) return;
    uint64_t t[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 4
    for (uint64_t p = blockIdx.z; p < n_problems; p += gridDim.z) {
        const SimView S = sim_view(batch, p);
        const uint32_t *d = diag + p * 2 * N;
        KinTable k;
        kin_pair_table(S, N, i, j, d[i], d[N + i], d[j], d[N + j], k);
#pragma unroll
        for (int c = 0; c < 9; ++c) t[c] += (uint64_t)k.t[c];
    }
    const uint64_t e = kin_pair_index(N, i, j) * 9;
    if (gridDim.z == 1) {
#pragma unroll
        for (int c = 0; c < 9; ++c) totals[e + c] += t[c];
    } else {
        uint64_t *o = part + (uint64_t)blockIdx.z * ((uint64_t)N * (N - 1) / 2 * 9) + e;
#pragma unroll
        for (int c = 0; c < 9; ++c) o[c] = t[c];
    }
}
__global__ __launch_bounds__(KIN_T) void kinship_totals_reduce_kernel(const uint64_t *__restrict__ part, uint64_t n_entries, uint32_t slices,
                                                                     uint64_t *__restrict__ totals) {
    const uint64_t e = (uint64_t)blockIdx.x * KIN_T + threadIdx.x;
    if (e >= n_entries) return;
    uint64_t v = 0;
    for (uint32_t z = 0; z < slices; ++z) v += part[(uint64_t)z * n_entries + e];
    totals[e] += v;
}

// slices of the totals kernel: enough (pair, slice) threads to fill the device, never more slices than windows
static uint32_t kinship_total_slices(uint32_t N, uint64_t n_problems) {
    const uint64_t pairs = (uint64_t)N * (N - 1) / 2;
    const uint64_t want = (KIN_TOTALS_THREADS + pairs - 1) / pairs;
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(want, KIN_TOTALS_MAX_SLICES), n_problems));
}

// window records and watch rows: one workgroup per problem
static int launch_kinship_windows(impop_ctx *ctx, const SimBatch &b, uint64_t n_problems, uint32_t N, int64_t num, int64_t den,
                           const uint32_t *d_watch, uint32_t n_watch, const KinshipOut &O) {
    if (!n_problems) return IMPOP_OK;
    REQUIRE(N >= 2 && N <= IMPOP_KINSHIP_MAX_N && 2 * N <= b.n && n_problems < 0x7FFFFFFFull && O.diag && (!n_watch || (d_watch && O.watch)),
            "launch_kinship_windows: bad shape");
    hipLaunchKernelGGL(kinship_window_kernel, dim3((uint32_t)n_problems), dim3(KIN_T), 0, ctx->stream, b, N, num, den, d_watch, n_watch, O,
                       O.diag, ctx->d_err);
    HIP_TRY(hipGetLastError());
    return IMPOP_OK;
}

// the per-pair tables of the chunk's problems added into O.totals: one thread per pair, the problems in turn
static int launch_kinship_totals(impop_ctx *ctx, const SimBatch &b, uint64_t n_problems, uint32_t N, const KinshipOut &O) {
    if (!n_problems) return IMPOP_OK;
    const uint32_t Z = kinship_total_slices(N, n_problems);
    REQUIRE(N >= 2 && N <= IMPOP_KINSHIP_MAX_N && 2 * N <= b.n && O.diag && O.totals && (Z == 1 || O.part), "launch_kinship_totals: bad shape");
    hipLaunchKernelGGL(kinship_totals_kernel, dim3((N - 1 + KIN_T - 1) / KIN_T, N - 1, Z), dim3(KIN_T), 0, ctx->stream, b, n_problems, N, O.diag,
                       O.totals, O.part);
    HIP_TRY(hipGetLastError());
    if (Z > 1) {
        const uint64_t n_entries = (uint64_t)N * (N - 1) / 2 * 9;
        hipLaunchKernelGGL(kinship_totals_reduce_kernel, dim3((uint32_t)((n_entries + KIN_T - 1) / KIN_T)), dim3(KIN_T), 0, ctx->stream, O.part,
                           n_entries, Z, O.totals);
        HIP_TRY(hipGetLastError());
    }
    return IMPOP_OK;
}

// impop_kinship_scan's epilogue: per chunk the window kernel (records, watch rows, the diagonals) and, when the per-pair totals are
// wanted, the totals kernel, which adds the chunk's tables into d_tot; d_tot lives across the chunks
struct KinshipEpilogue final : PairEpilogue {
    uint32_t N, n_watch;
    int64_t num, den;
    const uint32_t *watch;            // 2 x n_watch, host
    Result<impop_kin_window> win;
    Result<impop_kin_watch> wat;
    bool want_totals;
    uint64_t launches = 0;
    uint32_t *d_watch = nullptr, *d_diag = nullptr;
    uint64_t *d_tot = nullptr, *d_part = nullptr;
    size_t n_totals() const { return want_totals ? (size_t)N * (N - 1) / 2 * 9 : 0; }
    void layout(Layout &D, Layout &H, uint64_t cap) override {
        D.sub(d_watch, 2 * (size_t)n_watch); D.sub(d_tot, n_totals());
        const uint32_t Z = want_totals ? kinship_total_slices(N, cap) : 1u;  // the most slices a chunk of up to cap windows takes
        D.sub(d_part, Z > 1 ? Z * n_totals() : 0);
        D.sub(d_diag, cap * 2 * N); win.layout(D, H, cap); wat.layout(D, H, cap);
    }
    int upload(impop_ctx *ctx) override {
        if (n_watch) HIP_TRY(hipMemcpyAsync(d_watch, watch, 2 * (size_t)n_watch * 4, hipMemcpyHostToDevice, ctx->stream));
        if (want_totals) HIP_TRY(hipMemsetAsync(d_tot, 0, n_totals() * 8, ctx->stream));
        return IMPOP_OK;
    }
    int launch(impop_ctx *ctx, const PairChunk &c) override {
        // the epilogue kernels between two events of their own: impop_ctx_kinship_elapsed
        int rc = timed(ctx, ctx->timers[impop_ctx::T_KIN + 1], [&] {
            const KinshipOut O{win.d, n_watch ? wat.d : nullptr, want_totals ? d_tot : nullptr, d_diag, d_part};
            const int r = launch_kinship_windows(ctx, c.b, c.cnt, N, num, den, d_watch, n_watch, O);
            return r || !want_totals ? r : launch_kinship_totals(ctx, c.b, c.cnt, N, O);
        });
        if (rc) return rc;
        launches += !want_totals ? 1 : kinship_total_slices(N, c.cnt) > 1 ? 3 : 2;
        if ((rc = win.down(ctx, c.cnt))) return rc;
        return wat.down(ctx, c.cnt);
    }
    void collect(const PairChunk &c) override { win.scatter(c); wat.scatter(c); }
};

}  // namespace impop

using namespace impop;

IMPOP_API int impop_genotypes_create(impop_ctx *ctx, const impop_matrix *m, const uint32_t *pairs, uint32_t n_ind, impop_genotypes **out) {
    const char *fn = "impop_genotypes_create";
    REQUIRE(ctx && m && out, "%s: NULL argument", fn);
    *out = nullptr;
    REQUIRE(m->device == ctx->device, "%s: matrix lives on device %d, context on %d", fn, m->device, ctx->device);
    NOT_WEIGHTED(m, fn);
    REQUIRE(n_ind >= 2 && pairs, "%s: at least two individuals are needed", fn);
    if (n_ind > IMPOP_KINSHIP_MAX_N) {
        set_error("%s: %u individuals exceed the limit (%u)", fn, n_ind, (uint32_t)IMPOP_KINSHIP_MAX_N);
        return IMPOP_E_UNSUPPORTED;
    }
    const uint32_t n = m->g.n_hap, wps = m->g.wps, n_pad = wps * 32, N = n_ind;
    std::vector<int32_t> ppos(n_pad, -1);
    std::vector<uint32_t> pmask(wps, 0u);
    for (uint32_t i = 0; i < N; ++i) {
        const uint32_t h1 = pairs[2 * i], h2 = pairs[2 * i + 1];
        REQUIRE(h1 < n && h2 < n, "%s: individual %u: haplotype index %u outside the matrix's %u", fn, i, h1 < n ? h2 : h1, n);
        REQUIRE(h1 != h2, "%s: individual %u: both copies are haplotype %u", fn, i, h1);
        REQUIRE(ppos[h1] < 0 && ppos[h2] < 0, "%s: individual %u: haplotype %u is in two pairs", fn, i, ppos[h1] < 0 ? h2 : h1);
        ppos[h1] = (int32_t)(2 * i);
        ppos[h2] = (int32_t)(2 * i + 1);
        pmask[h1 >> 5] |= 1u << (h1 & 31);
        pmask[h2 >> 5] |= 1u << (h2 & 31);
    }
    REQUIRE((m->g.n_block + 3) / 4 < 0x7FFFFFFFull, "%s: matrix too long for one launch", fn);
    HIP_TRY(hipSetDevice(ctx->device));

    // the wrapped matrix: geometry of 2N rows over the source's sites, the RB32 operand and nothing else
    impop_matrix *p = new impop_matrix();
    auto fail = [&](int code) {
        impop_matrix_free(ctx, p);
        return code;
    };
    p->g.n_hap = 2 * N; p->g.wps = (2 * N + 31) / 32; p->g.G = (p->g.wps + 3) / 4; p->g.r = p->g.wps - 4 * (p->g.G - 1);
    p->g.n_site = m->g.n_site; p->g.n_block = m->g.n_block;
    p->device = ctx->device;
    p->n_hap_pad = (2 * N + 95) / 96 * 96;
    p->phi_row = 0xFFFFFFFFu;  // the planes are sparse as given
    p->rb_nb = p->g.n_block + 8;
    p->rb_bytes = (uint64_t)(p->n_hap_pad / 32) * p->rb_nb * 32ull * 8ull;
    p->vskip = p->rskip = p->sskip = p->uskip = "genotype planes";
    hipError_t e = hipMalloc((void **)&p->d_rb, p->rb_bytes);
    if (e != hipSuccess) return fail(hip_fail(e, "hipMalloc(genotype planes)", __FILE__, __LINE__));
    if ((e = hipMemsetAsync(p->d_rb, 0, p->rb_bytes, ctx->stream)) != hipSuccess) return fail(hip_fail(e, "hipMemsetAsync", __FILE__, __LINE__));
    if (m->compact) {  // the planes' sites are the source's kept sites
        p->compact = true;
        p->n_site_orig = m->n_site_orig;
        p->pos = m->pos;
        p->pos_coarse = m->pos_coarse;
        const size_t ones_bytes = (size_t)((m->n_site_orig + 63) / 64) * 8 + 256;  // as impop_matrix_compact allocated it
        if (m->d_onesmap && m->n_site_orig) {
            if ((e = hipMalloc((void **)&p->d_onesmap, ones_bytes)) != hipSuccess) return fail(hip_fail(e, "hipMalloc(all-ones bitmap)", __FILE__, __LINE__));
            if ((e = hipMemcpyAsync(p->d_onesmap, m->d_onesmap, ones_bytes - 256, hipMemcpyDeviceToDevice, ctx->stream)) != hipSuccess)
                return fail(hip_fail(e, "hipMemcpyAsync(all-ones bitmap)", __FILE__, __LINE__));
            if ((e = hipMemsetAsync((char *)p->d_onesmap + ones_bytes - 256, 0, 256, ctx->stream)) != hipSuccess)
                return fail(hip_fail(e, "hipMemsetAsync", __FILE__, __LINE__));
        }
        if (m->d_pos && !m->pos.empty()) {
            if ((e = hipMalloc((void **)&p->d_pos, m->pos.size() * 8)) != hipSuccess) return fail(hip_fail(e, "hipMalloc(positions)", __FILE__, __LINE__));
            if ((e = hipMemcpyAsync(p->d_pos, m->d_pos, m->pos.size() * 8, hipMemcpyDeviceToDevice, ctx->stream)) != hipSuccess)
                return fail(hip_fail(e, "hipMemcpyAsync(positions)", __FILE__, __LINE__));
        }
    }
    if (m->g.n_block) {
        Carve L;
        const size_t o_ppos = L.take<int32_t>(n_pad), o_pmask = L.take<uint32_t>(wps);
        void *d = nullptr;
        int rc = ctx_scratch(ctx, L.total(), &d);
        if (rc) return fail(rc);
        // pageable sources: the copies are staged by the runtime before they return
        if ((e = hipMemcpyAsync(L.at<int32_t>(d, o_ppos), ppos.data(), (size_t)n_pad * 4, hipMemcpyHostToDevice, ctx->stream)) != hipSuccess ||
            (e = hipMemcpyAsync(L.at<uint32_t>(d, o_pmask), pmask.data(), (size_t)wps * 4, hipMemcpyHostToDevice, ctx->stream)) != hipSuccess)
            return fail(hip_fail(e, "hipMemcpyAsync(pairs)", __FILE__, __LINE__));
        // waves of a workgroup: as many of 4 as the LDS holds words for (N <= 1024: 4, N = 2048: 2)
        const size_t lds_wave = (size_t)2 * N * 8;
        const uint32_t n_waves = (uint32_t)std::max<size_t>(1, std::min<size_t>(4, GENO_LDS_BUDGET / lds_wave));
        const size_t lds = lds_wave * n_waves;
        if ((rc = lds_opt_in(geno_planes_kernel, lds))) return fail(rc);
        const uint64_t grid = (m->g.n_block + n_waves - 1) / n_waves;
        if (grid >= 0x7FFFFFFFull) {
            set_error("%s: matrix too long for one launch", fn);
            return fail(IMPOP_E_INVALID);
        }
        rc = timed(ctx, ctx->timers[impop_ctx::T_KIN], [&] {
            hipLaunchKernelGGL(geno_planes_kernel, dim3((uint32_t)grid), dim3(64 * n_waves), lds, ctx->stream, m->d_sb, wps, m->g.G, m->g.r,
                               m->g.n_block, m->g.n_site, L.at<int32_t>(d, o_ppos), L.at<uint32_t>(d, o_pmask), N, p->d_rb, p->rb_nb);
        });
        if (rc) return fail(rc);
    }
    if ((e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return fail(hip_fail(e, "hipStreamSynchronize", __FILE__, __LINE__));
    impop_genotypes *g = new impop_genotypes();
    g->planes = p;
    g->n_ind = N;
    *out = g;
    return IMPOP_OK;
}

IMPOP_API int impop_genotypes_info(const impop_genotypes *g, uint32_t *n_ind, uint64_t *n_site, uint64_t *device_bytes) {
    REQUIRE(g && g->planes, "impop_genotypes_info: genotypes is NULL");
    if (n_ind) *n_ind = g->n_ind;
    if (n_site) *n_site = g->planes->g.n_site;
    if (device_bytes) *device_bytes = g->planes->rb_bytes;
    return IMPOP_OK;
}

IMPOP_API int impop_genotypes_download(impop_ctx *ctx, const impop_genotypes *g, uint64_t site_begin, uint64_t site_end,
                                       uint64_t *bits_row_major, uint64_t row_stride_words) {
    const char *fn = "impop_genotypes_download";
    REQUIRE(ctx && g && g->planes, "%s: NULL argument", fn);
    const impop_matrix *p = g->planes;
    REQUIRE(site_begin <= site_end && site_end <= p->g.n_site, "%s: bad site range [%llu,%llu)", fn, (unsigned long long)site_begin,
            (unsigned long long)site_end);
    const uint64_t nw = (site_end - site_begin + 63) / 64;
    if (!nw) return IMPOP_OK;
    REQUIRE(bits_row_major && row_stride_words >= nw, "%s: NULL output or a row stride below %llu words", fn, (unsigned long long)nw);
    const uint32_t rows = 2 * g->n_ind;
    const uint64_t total = (uint64_t)rows * nw;
    REQUIRE((total + 255) / 256 < 0x7FFFFFFFull, "%s: range too long for one launch", fn);
    HIP_TRY(hipSetDevice(ctx->device));
    void *d = nullptr;
    int rc = ctx_scratch(ctx, total * 8, &d);
    if (rc) return rc;
    hipLaunchKernelGGL(geno_download_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, ctx->stream, p->d_rb, p->rb_nb, rows,
                       site_begin, site_end, nw, (uint64_t *)d);
    HIP_TRY(hipGetLastError());
    std::vector<uint64_t> h(total);
    HIP_TRY(hipMemcpyAsync(h.data(), d, total * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (uint32_t r = 0; r < rows; ++r) memcpy(bits_row_major + (uint64_t)r * row_stride_words, h.data() + (uint64_t)r * nw, nw * 8);
    return IMPOP_OK;
}

IMPOP_API int impop_genotypes_free(impop_ctx *ctx, impop_genotypes *g) {
    if (!g) return IMPOP_OK;
    const int rc = impop_matrix_free(ctx, g->planes);
    if (rc) return rc;
    delete g;
    return IMPOP_OK;
}

static_assert(sizeof(impop_kin_window) == 48 && sizeof(impop_kin_pair) == 72 && sizeof(impop_kin_watch) == 16 &&
                  sizeof(impop_kinship_params) == 16, "fixed record layouts");

IMPOP_API int impop_kinship_scan(impop_ctx *ctx, const impop_genotypes *g, const impop_window *windows, uint64_t n_windows,
                                 const impop_kinship_params *params, const uint32_t *watch, uint32_t n_watch,
                                 impop_kin_window *out_windows, impop_kin_pair *out_pairs, impop_kin_watch *out_watch) {
    const char *fn = "impop_kinship_scan";
    REQUIRE(ctx && g && g->planes && params, "%s: NULL argument", fn);
    REQUIRE(params->struct_size == sizeof(impop_kinship_params), "impop_kinship_params.struct_size mismatch");
    REQUIRE(params->kin_den >= 1 && params->kin_den <= (1u << 20) && params->kin_num <= params->kin_den,
            "%s: the threshold kin_num / kin_den needs 1 <= kin_den <= 2^20 and kin_num <= kin_den", fn);
    const impop_matrix *m = g->planes;
    const uint32_t N = g->n_ind;
    REQUIRE(m->device == ctx->device, "%s: genotypes live on device %d, context on %d", fn, m->device, ctx->device);
    REQUIRE(n_watch <= IMPOP_KINSHIP_MAX_WATCH, "%s: %u watched pairs exceed the limit (%u)", fn, n_watch, (uint32_t)IMPOP_KINSHIP_MAX_WATCH);
    REQUIRE(!n_watch || (watch && out_watch), "%s: NULL watch / out_watch with n_watch = %u", fn, n_watch);
    for (uint32_t q = 0; q < n_watch; ++q) {
        const uint32_t a = watch[2 * q], b = watch[2 * q + 1];
        REQUIRE(a < N && b < N, "%s: watched pair %u: individual %u outside the handle's %u", fn, q, a < N ? b : a, N);
        REQUIRE(a != b, "%s: watched pair %u names individual %u twice", fn, q, a);
    }
    bool go;
    int rc = windows_ready(ctx, m, windows, n_windows, out_windows, fn, &go);
    if (rc || !go) return rc;
    KinshipEpilogue epi;
    epi.N = N; epi.n_watch = n_watch; epi.num = params->kin_num; epi.den = params->kin_den;
    epi.watch = watch; epi.want_totals = out_pairs != nullptr;
    epi.win.want(out_windows, 1); epi.wat.want(out_watch, n_watch);
    PairFront in = hamming_front(fn, widest_W(m, windows, n_windows));  // no polarity row: the counts are used as written
    rc = pairwise_front(ctx, m, windows, n_windows, in, epi);
    if (rc) return rc;
    if (out_pairs) {  // the scratch the front end bound the totals into is still the context's
        HIP_TRY(hipMemcpyAsync(out_pairs, epi.d_tot, epi.n_totals() * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    if (trace_on())
        fprintf(stderr, "[impop_kinship_scan] route=%s individuals=%u rows=%u windows=%llu chunks=%llu launches=%llu watch=%u plane_bytes=%llu\n",
                m->compact ? "compact" : "dense", N, m->n_hap_pad, (unsigned long long)n_windows, (unsigned long long)in.chunks,
                (unsigned long long)epi.launches, n_watch, (unsigned long long)m->rb_bytes);
    return IMPOP_OK;
}
