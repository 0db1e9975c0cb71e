// stats_batch.hip — pica2 / h-fst / Tajima's D on a RAGGED batch of dense identity matrices: one `.sim` table per window
// (run_pica2_impg.sh:162-175, run_h-fst.sh:65-81, run_tajd.sh:160-180), every table with its own size, seed order and
// population flags.  The kernels of stats.hip take a SimBatch that is uniform over the batch; here every workgroup reads its
// problem from a descriptor table on the device.  Per chunk of tables: one upload of the matrices, one of the side tables
// (descriptors, seed orders, flags), two launches whatever the number of tables, one download of records + group indices.
//
// Why the grouping is not stats.hip's greedy_groups: that function (and the blocked bit form behind it) is shaped for Gram
// problems of up to 8192 elements and lives next to the kernels whose code it is tuned with; a dense problem of at most 1023
// elements needs none of it.  A seed's whole row is four loads per thread, issued together before the first is used
// (no branch on a runtime value around a load), and a group costs two barriers.  Same decisions: strict `>` on the
// rounded identity, seeds in the handed-in order or by smallest remaining index, groups renumbered by smallest member.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "stats_kernels.h"

namespace impop {

namespace {

constexpr uint32_t BNONE = 0xFFFFFFFFu;
constexpr int BT = 256;               // threads per problem
constexpr uint32_t BATCH_MAX_N = 1023;  // one workgroup per problem, no row split
constexpr uint32_t BN = 1024;           // LDS arrays per problem
constexpr int ROW_U = BN / BT;          // loads per thread that cover a row

struct BatchDesc {  // 64 bytes, one per problem of a chunk
    uint64_t mat_off;    // element offset of the n x n matrix in the chunk's matrix buffer
    uint64_t seq_len;    // 0 = None
    uint32_t n;
    uint32_t order_off;  // seed order (positions, n entries) in the u32 side table, BNONE = by smallest remaining index
    uint32_t flag_off;   // in_a (n bytes) then in_b (n bytes) in the flag table, BNONE = no Fst fields
    uint32_t grp_off;    // first of the problem's n group indices in the output
    int64_t taj_n;       // < 2: no D
    double taj_S;
    uint64_t pad[2];
};
static_assert(sizeof(BatchDesc) == 64, "descriptor layout");
static_assert(sizeof(impop_identity_stats) == IMPOP_IDENTITY_STATS_BYTES, "record layout is part of the ABI");

__device__ __forceinline__ uint32_t wave_id() { return (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

__device__ __forceinline__ SimView dense_view(const double *mat, uint32_t n, int round_digits) {
    SimView S;
    S.dense = mat; S.gram = nullptr; S.ld = n; S.W = 0; S.kind = 0; S.round_digits = round_digits;
    S.tbl = nullptr; S.tbl_n = 0; S.diag = nullptr; S.nseg = 1; S.seg_stride = 0; S.add = 0; S.err = nullptr; S.g16 = 0;
    return S;
}

// Tajima's D the way run_tajd.sh:174-180 wires it: pica2's pi per site through its "%.8f" text into tj_d.py -p; NaN where
// tj_d.py would refuse the arguments (tj_d.py:48-51) or pica2 printed no per-site value
__host__ __device__ inline double tajima_d_from_pi_site(int64_t n, double S, double pi_site) {
    if (!(n >= 2 && S >= 0 && pi_site >= 0)) return __builtin_nan("");
    return tajima_d_from(tajima_consts(n), S, py_round(pi_site, 8), nullptr, nullptr);
}

// pica2.analyze_similarity_matrix (pica2.py:60-169) on problem blockIdx.x, then Tajima's D from the "%.8f" text of pi per site
// (run_tajd.sh:174-180).  Writes the whole record (Fst fields: "none"; hfst_batch_kernel fills them where flags were given).
__global__ __launch_bounds__(BT) void pica2_batch_kernel(const BatchDesc *__restrict__ descs, const double *__restrict__ mats,
                                                        const uint32_t *__restrict__ u32tab, double threshold, int round_digits,
                                                        impop_identity_stats *__restrict__ out, uint32_t *__restrict__ group_of,
                                                        uint32_t *err) {
    __shared__ uint32_t grp[BN], gsz[BN], rep[BN], gmin[BN], newid[BN];
    __shared__ double rowsum[BN];
    __shared__ uint32_t chunk_cnt[BT];
    __shared__ uint32_t sh_have;
    __shared__ unsigned long long sh_npairs;
    const BatchDesc d = descs[blockIdx.x];
    const uint32_t n = d.n, tid = threadIdx.x;
    const double *mat = mats + d.mat_off;
    const uint32_t *order = d.order_off != BNONE ? u32tab + d.order_off : nullptr;
    const SimView S = dense_view(mat, n, round_digits);
    for (uint32_t i = tid; i < BN; i += BT) { grp[i] = BNONE; gsz[i] = 0; }
    if (tid == 0) { sh_have = 0; sh_npairs = 0; }
    __syncthreads();
    // Step 1 (pica2.py:94-112)
    uint32_t G = 0;
    const uint32_t last = n ? n - 1 : 0;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t seed = order ? order[k] : k;
        if (grp[seed] != BNONE) continue;  // uniform across the workgroup
        const double *row = mat + (uint64_t)seed * n;
        double sv[ROW_U];
#pragma unroll
        for (int u = 0; u < ROW_U; ++u) {  // the seed's whole row, in flight together (positions past n re-read the last entry)
            const uint32_t o = tid + (uint32_t)u * BT;
            sv[u] = row[o < n ? o : last];
        }
        uint32_t cnt = 0;
#pragma unroll
        for (int u = 0; u < ROW_U; ++u) {
            const uint32_t o = tid + (uint32_t)u * BT;
            double v = sv[u];
            if (round_digits >= 0 && v == v) v = py_round(v, round_digits);
            if (o < n && o != seed && grp[o] == BNONE && v == v && v > threshold) { grp[o] = G; ++cnt; }  // strict > (pica2.py:106)
        }
        __syncthreads();  // every thread has tested grp[seed] and its own candidates before the seed is marked
        if (tid == 0) { grp[seed] = G; ++cnt; rep[G] = seed; }
        if (cnt) atomicAdd(&gsz[G], cnt);
        ++G;
        __syncthreads();
    }
    if (order) {  // renumber by smallest member (pica2.py:110-112: sorted(group), groups.sort())
        for (uint32_t g = tid; g < G; g += BT) gmin[g] = BNONE;
        __syncthreads();
        for (uint32_t i = tid; i < n; i += BT) atomicMin(&gmin[grp[i]], i);
        __syncthreads();
        const uint32_t per = (n + BT - 1) / BT, lo = tid * per < n ? tid * per : n, hi = lo + per < n ? lo + per : n;
        uint32_t c = 0;
        for (uint32_t i = lo; i < hi; ++i) c += gmin[grp[i]] == i;
        chunk_cnt[tid] = c;
        __syncthreads();
        uint32_t base = 0;
        for (uint32_t t = 0; t < tid; ++t) base += chunk_cnt[t];
        for (uint32_t i = lo; i < hi; ++i)
            if (gmin[grp[i]] == i) newid[grp[i]] = base++;
        __syncthreads();
        for (uint32_t i = tid; i < n; i += BT) grp[i] = newid[grp[i]];
        for (uint32_t g = tid; g < G; g += BT) gsz[g] = 0;
        __syncthreads();
        for (uint32_t i = tid; i < n; i += BT) atomicAdd(&gsz[grp[i]], 1u);
        for (uint32_t g = tid; g < G; g += BT) rep[newid[g]] = gmin[g];
        __syncthreads();
    }
    {  // every element sits in exactly one group
        uint32_t tot = 0;
        for (uint32_t g = tid; g < G; g += BT) tot += gsz[g];
        tot = (uint32_t)block_sum_u64_n<BT>(tot, reinterpret_cast<uint64_t *>(rowsum));
        if (tot != n && tid == 0 && err) atomicOr(err, DEV_ERR_GROUPING);
        __syncthreads();
    }
    // Step 2-3 (pica2.py:118-154): sum over group pairs of 2 (1 - sim(rep_i, rep_j)) f_i f_j
    const double total = (double)n;
    uint32_t have = 0;
    uint64_t npairs = 0;
    if (G <= 64) {  // few groups (the usual case): a thread per row, the row's pairs in the reference's order
        for (uint32_t i = tid; i < G; i += BT) {
            const double fi = (double)gsz[i] / total;
            double acc = 0.0;
            for (uint32_t j = i + 1; j < G; ++j) {
                const double s = sim_get(S, rep[i], rep[j]);
                if (s != s) continue;  // missing pair skipped (pica2.py:132-134)
                const double fj = (double)gsz[j] / total;
                acc += 2 * ((1 - s) * fi * fj);
                have = 1;
                ++npairs;
            }
            rowsum[i] = acc;
        }
    } else {  // many groups: a wave per row, lanes along it; the raw identities of eight columns are loaded before any is rounded
        const uint32_t lane = tid & 63;
        constexpr int P2_U = 8;
        for (uint32_t i = wave_id(); i < G; i += BT / 64) {
            const uint32_t ri = rep[i];
            const double fi = (double)gsz[i] / total;
            double acc = 0.0;
            for (uint32_t j0 = i + 1 + lane; j0 < G; j0 += 64 * P2_U) {
                double sv[P2_U];
#pragma unroll
                for (int u = 0; u < P2_U; ++u) {
                    const uint32_t j = j0 + 64 * u;
                    const uint32_t rj = rep[j < G ? j : i];  // past the end: the diagonal entry, dropped below
                    sv[u] = mat[(uint64_t)(ri < rj ? ri : rj) * n + (ri < rj ? rj : ri)];  // the pair's key, as sim_get reads it
                }
#pragma unroll
                for (int u = 0; u < P2_U; ++u) {
                    const uint32_t j = j0 + 64 * u;
                    double s = sv[u];
                    if (j >= G || s != s) continue;  // missing pair skipped (pica2.py:132-134)
                    if (round_digits >= 0) s = py_round(s, round_digits);
                    const double fj = (double)gsz[j] / total;
                    acc += 2 * ((1 - s) * fi * fj);
                    have = 1;
                    ++npairs;
                }
            }
            acc = wave_sum_f64(acc);
            if (lane == 0) rowsum[i] = acc;
        }
    }
    if (have) atomicOr(&sh_have, 1u);
    if (npairs) atomicAdd(&sh_npairs, (unsigned long long)npairs);
    __syncthreads();
    if (tid == 0) {
        double acc = 0.0;
        for (uint32_t i = 0; i < G; ++i) acc += rowsum[i];
        double pi = 0.0, pi_site = 0.0;  // the degenerate returns of pica2.py:122-124, 150-152
        if (n != 0 && sh_have) {
            pi = ((double)n / (double)(n - 1)) * acc;                              // pica2.py:154
            pi_site = d.seq_len ? pi / (double)d.seq_len : __builtin_nan("");      // :163-164, None -> NaN
        }
        const double nan = __builtin_nan("");
        impop_identity_stats o;
        o.status = IMPOP_OK; o.n_groups = G;
        o.pi = pi; o.pi_site = pi_site; o.sum_2pairs = acc; o.n_pairs_with_data = sh_npairs;
        for (int k = 0; k < 6; ++k) { o.fst[k] = nan; o.fst_counts[k] = 0; }
        o.tajima_d = tajima_d_from_pi_site(d.taj_n, d.taj_S, pi_site);
        out[blockIdx.x] = o;
    }
    for (uint32_t i = tid; i < n; i += BT) group_of[d.grp_off + i] = grp[i];
}

// h-fst.calculate_fst (h-fst.py:173-249) on problem blockIdx.x (problems without flags: nothing to do).  Rows, lanes and the order
// of every thread's additions are those of hfst_kernel's dense branch (stats.hip), four columns in flight per lane.
__global__ __launch_bounds__(BT) void hfst_batch_kernel(const BatchDesc *__restrict__ descs, const double *__restrict__ mats,
                                                       const uint8_t *__restrict__ flags, int round_digits,
                                                       impop_identity_stats *__restrict__ out) {
    __shared__ uint8_t cls[BN];
    __shared__ double shd[BT / 64];
    __shared__ uint64_t shu[BT / 64];
    const BatchDesc d = descs[blockIdx.x];
    if (d.flag_off == BNONE) return;  // uniform
    const uint32_t n = d.n, tid = threadIdx.x, lane = tid & 63;
    const double *mat = mats + d.mat_off;
    const uint8_t *in_a = flags + d.flag_off, *in_b = in_a + n;
    for (uint32_t i = tid; i < BN; i += BT) {  // 1 = A only, 2 = B only, 0 = neither or both (h-fst.py:181-185)
        const bool a = i < n && in_a[i], b = i < n && in_b[i];
        cls[i] = (a && !b) ? 1 : (b && !a) ? 2 : 0;
    }
    __syncthreads();
    double accA = 0.0, accB = 0.0, accX = 0.0;
    uint64_t cA = 0, mA = 0, cB = 0, mB = 0, cX = 0, mX = 0;
    const uint32_t last = n ? n - 1 : 0;
    constexpr int HU = 4;
    for (uint32_t r = wave_id(); r < n; r += BT / 64) {
        const uint32_t cr = cls[r];  // wave-uniform
        if (!cr) continue;
        const double *row = mat + (uint64_t)r * n;
        for (uint32_t c0 = r + 1 + lane; c0 < n; c0 += 64 * HU) {
            double sv[HU];
#pragma unroll
            for (int u = 0; u < HU; ++u) {
                const uint32_t c = c0 + 64 * u;
                sv[u] = row[c < n ? c : last];
            }
#pragma unroll
            for (int u = 0; u < HU; ++u) {
                const uint32_t c = c0 + 64 * u;
                const uint32_t cc = c < n ? cls[c] : 0u;
                if (!cc) continue;
                double s = sv[u];
                if (round_digits >= 0 && s == s) s = py_round(s, round_digits);
                const bool miss = s != s;
                const double dd = 1 - s;
                if (cr != cc) { if (miss) ++mX; else { accX += dd; ++cX; } }
                else if (cr == 1) { if (miss) ++mA; else { accA += dd; ++cA; } }
                else { if (miss) ++mB; else { accB += dd; ++cB; } }
            }
        }
    }
    accA = block_sum_f64_n<BT>(accA, shd); accB = block_sum_f64_n<BT>(accB, shd); accX = block_sum_f64_n<BT>(accX, shd);
    cA = block_sum_u64_n<BT>(cA, shu); mA = block_sum_u64_n<BT>(mA, shu);
    cB = block_sum_u64_n<BT>(cB, shu); mB = block_sum_u64_n<BT>(mB, shu);
    cX = block_sum_u64_n<BT>(cX, shu); mX = block_sum_u64_n<BT>(mX, shu);
    if (tid == 0) {
        HfstOut o;
        hfst_outputs(accA, accB, accX, cA, mA, cB, mB, cX, mX, d.seq_len, &o);
        for (int k = 0; k < 6; ++k) { out[blockIdx.x].fst[k] = o.v[k]; out[blockIdx.x].fst_counts[k] = o.cnt[k]; }
    }
}

struct ChunkLayout {  // one device (and one pinned host) allocation per chunk, every part on a 256-byte boundary
    size_t mats, descs, u32tab, flags, recs, groups, total;
    size_t side_bytes() const { return recs - descs; }  // descriptors + seed orders + flags: the second upload
    size_t down_bytes() const { return total - recs; }  // records + group indices: the download
};
ChunkLayout chunk_layout(size_t mat_el, size_t k, size_t n_order, size_t n_flag, size_t n_grp) {
    Carve cv;
    ChunkLayout L;
    L.mats = cv.take<double>(mat_el);
    L.descs = cv.take<BatchDesc>(k);
    L.u32tab = cv.take<uint32_t>(n_order);
    L.flags = cv.take<uint8_t>(n_flag);
    L.recs = cv.take<impop_identity_stats>(k);
    L.groups = cv.take<uint32_t>(n_grp);
    L.total = cv.total();
    return L;
}

}  // namespace
}  // namespace impop

using namespace impop;

// the batch kernels' Tajima wiring as host arithmetic (no device): what a record's tajima_d holds for (n, S, pi_site)
IMPOP_API int impop_tajimas_d_from_pi_site(int64_t n, double S, double pi_site, double *D) {
    REQUIRE(D, "impop_tajimas_d_from_pi_site: D is NULL");
    *D = tajima_d_from_pi_site(n, S, pi_site);
    return IMPOP_OK;
}

IMPOP_API int impop_stats_from_identity_batch(impop_ctx *ctx, const impop_identity_problem *problems, uint64_t k,
                                              const impop_identity_batch_params *params, impop_identity_stats *out,
                                              uint32_t *group_of) {
    REQUIRE(ctx, "impop_stats_from_identity_batch: ctx is NULL");
    if (!k) return IMPOP_OK;
    REQUIRE(problems && out, "impop_stats_from_identity_batch: NULL argument");
    impop_identity_batch_params P;
    P.struct_size = sizeof P; P.threshold = 1.0; P.round_digits = -1; P.fst_round_digits = -1; P.max_chunk_bytes = 0;
    if (params) {
        REQUIRE(params->struct_size >= 4 && params->struct_size <= sizeof P, "impop_stats_from_identity_batch: bad params.struct_size");
        memcpy(&P, params, params->struct_size);
    }
    REQUIRE(P.round_digits <= 19 && P.fst_round_digits <= 19, "impop_stats_from_identity_batch: round digits > 19 unsupported");
    const int rd = P.round_digits < 0 ? -1 : P.round_digits, frd = P.fst_round_digits < 0 ? -1 : P.fst_round_digits;
    for (uint64_t p = 0; p < k; ++p) {
        const impop_identity_problem &q = problems[p];
        REQUIRE(q.n == 0 || q.ident, "impop_stats_from_identity_batch: problem %llu: ident is NULL", (unsigned long long)p);
        REQUIRE((q.in_a != nullptr) == (q.in_b != nullptr), "impop_stats_from_identity_batch: problem %llu: in_a and in_b go together",
                (unsigned long long)p);
    }
    HIP_TRY(hipSetDevice(ctx->device));
    // chunks are capped by the bytes they upload; default: what the context's scratch already holds, at least 128 MiB
    const size_t cap = P.max_chunk_bytes ? (size_t)P.max_chunk_bytes : std::max<size_t>(ctx->scratch_bytes, (size_t)128 << 20);
    const bool trace = trace_on();
    std::vector<uint64_t> grp_base(k + 1, 0);  // where each problem's group indices start in the caller's array
    for (uint64_t p = 0; p < k; ++p) grp_base[p + 1] = grp_base[p] + problems[p].n;
    std::vector<uint32_t> order;
    uint32_t chunk_no = 0;
    // IMPOP_TRACE=1 only: events around the chunk's uploads, kernels and download (tools/bench_sim_list.py reads the split)
    struct TraceEvents {
        hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
        ~TraceEvents() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    } tev;
    if (trace)
        for (hipEvent_t &x : tev.e) HIP_TRY(hipEventCreate(&x));
    for (uint64_t p0 = 0; p0 < k;) {
        // the chunk [p0, p1): supported problems until the byte cap (a chunk holds at least one)
        uint64_t p1 = p0;
        size_t mat_el = 0, n_order = 0, n_flag = 0, n_grp = 0, n_in = 0, bytes = 0;
        uint32_t max_n = 0;
        for (; p1 < k; ++p1) {
            const impop_identity_problem &q = problems[p1];
            if (q.n > BATCH_MAX_N) continue;
            const size_t add = (size_t)q.n * q.n * 8 + sizeof(BatchDesc) + (q.seed_rank ? (size_t)q.n * 4 : 0) + (q.in_a ? 2 * (size_t)q.n : 0);
            if (n_in && bytes + add > cap) break;
            bytes += add;
            mat_el += (size_t)q.n * q.n; n_order += q.seed_rank ? q.n : 0; n_flag += q.in_a ? 2 * (size_t)q.n : 0; n_grp += q.n;
            max_n = std::max(max_n, q.n);
            ++n_in;
        }
        for (uint64_t p = p0; p < p1; ++p)  // a larger problem: its own status, through the single-problem entry points if wanted
            if (problems[p].n > BATCH_MAX_N) {
                memset(&out[p], 0, sizeof out[p]);
                out[p].status = IMPOP_E_UNSUPPORTED;
                if (group_of) memset(group_of + grp_base[p], 0, (size_t)problems[p].n * 4);
            }
        if (!n_in) { p0 = p1; continue; }
        REQUIRE(n_order < 0xFFFFFFFFull && n_flag < 0xFFFFFFFFull && n_grp < 0xFFFFFFFFull, "impop_stats_from_identity_batch: chunk too large");
        const ChunkLayout L = chunk_layout(mat_el, n_in, n_order, n_flag, n_grp);
        void *hp = nullptr, *dp = nullptr;
        int rc = ctx_pinned(ctx, L.total, &hp);
        if (rc) return rc;
        rc = ctx_scratch(ctx, L.total, &dp);
        if (rc) return rc;
        char *h = (char *)hp, *dv = (char *)dp;
        double *h_mats = reinterpret_cast<double *>(h + L.mats);
        BatchDesc *h_desc = reinterpret_cast<BatchDesc *>(h + L.descs);
        uint32_t *h_u32 = reinterpret_cast<uint32_t *>(h + L.u32tab);
        uint8_t *h_flags = reinterpret_cast<uint8_t *>(h + L.flags);
        size_t mo = 0, oo = 0, fo = 0, go = 0, s = 0;
        const auto t_stage = std::chrono::steady_clock::now();
        for (uint64_t p = p0; p < p1; ++p) {
            const impop_identity_problem &q = problems[p];
            if (q.n > BATCH_MAX_N) continue;
            BatchDesc d{};
            d.mat_off = mo; d.seq_len = q.seq_len; d.n = q.n; d.order_off = BNONE; d.flag_off = BNONE; d.grp_off = (uint32_t)go;
            d.taj_n = q.tajima_n; d.taj_S = q.tajima_S;
            const size_t nn = (size_t)q.n * q.n;
            if (nn) memcpy(h_mats + mo, q.ident, nn * 8);
            if (q.seed_rank && q.n) {  // seed_rank -> order (inverse permutation); ranks must be distinct
                uint32_t dup = 0;
                REQUIRE(seed_order_of(q.seed_rank, nullptr, q.n, order, &dup) == IMPOP_OK,
                        "impop_stats_from_identity_batch: problem %llu: seed_rank must be distinct (rank %u occurs twice)",
                        (unsigned long long)p, dup);
                memcpy(h_u32 + oo, order.data(), (size_t)q.n * 4);
                d.order_off = (uint32_t)oo;
                oo += q.n;
            }
            if (q.in_a) {
                if (q.n) { memcpy(h_flags + fo, q.in_a, q.n); memcpy(h_flags + fo + q.n, q.in_b, q.n); }
                d.flag_off = (uint32_t)fo;
                fo += 2 * (size_t)q.n;
            }
            h_desc[s++] = d;
            mo += nn; go += q.n;
        }
        const long long stage_us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t_stage).count();
        if (trace) HIP_TRY(hipEventRecord(tev.e[0], ctx->stream));
        if (mat_el) HIP_TRY(hipMemcpyAsync(dv + L.mats, h + L.mats, mat_el * 8, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(dv + L.descs, h + L.descs, L.side_bytes(), hipMemcpyHostToDevice, ctx->stream));
        const BatchDesc *d_desc = reinterpret_cast<const BatchDesc *>(dv + L.descs);
        const double *d_mats = reinterpret_cast<const double *>(dv + L.mats);
        impop_identity_stats *d_recs = reinterpret_cast<impop_identity_stats *>(dv + L.recs);
        uint32_t launches = 0;
        if (trace) HIP_TRY(hipEventRecord(tev.e[1], ctx->stream));
        hipLaunchKernelGGL(pica2_batch_kernel, dim3((uint32_t)n_in), dim3(BT), 0, ctx->stream, d_desc, d_mats,
                           reinterpret_cast<const uint32_t *>(dv + L.u32tab), P.threshold, rd, d_recs,
                           reinterpret_cast<uint32_t *>(dv + L.groups), ctx->d_err);
        HIP_TRY(hipGetLastError());
        ++launches;
        hipLaunchKernelGGL(hfst_batch_kernel, dim3((uint32_t)n_in), dim3(BT), 0, ctx->stream, d_desc, d_mats,
                           reinterpret_cast<const uint8_t *>(dv + L.flags), frd, d_recs);
        HIP_TRY(hipGetLastError());
        ++launches;
        if (trace) HIP_TRY(hipEventRecord(tev.e[2], ctx->stream));
        HIP_TRY(hipMemcpyAsync(h + L.recs, dv + L.recs, L.down_bytes(), hipMemcpyDeviceToHost, ctx->stream));
        if (trace) HIP_TRY(hipEventRecord(tev.e[3], ctx->stream));
        rc = ctx_err_fetch(ctx);
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        rc = ctx_err_result(ctx, "impop_stats_from_identity_batch");
        if (rc) return rc;
        const impop_identity_stats *h_recs = reinterpret_cast<const impop_identity_stats *>(h + L.recs);
        const uint32_t *h_grp = reinterpret_cast<const uint32_t *>(h + L.groups);
        s = 0; go = 0;
        for (uint64_t p = p0; p < p1; ++p) {
            const impop_identity_problem &q = problems[p];
            if (q.n > BATCH_MAX_N) continue;
            out[p] = h_recs[s++];
            if (group_of && q.n) memcpy(group_of + grp_base[p], h_grp + go, (size_t)q.n * 4);
            go += q.n;
        }
        if (trace) {  // stage = host copy into the page-locked buffer; up / kernels / down = GPU time between events
            float ms[3] = {0.f, 0.f, 0.f};
            for (int i = 0; i < 3; ++i) HIP_TRY(hipEventElapsedTime(&ms[i], tev.e[i], tev.e[i + 1]));
            fprintf(stderr, "[impop_sim_batch] tables=%zu chunk=%u bytes_up=%zu launches=%u max_n=%u stage_us=%lld up_us=%lld kernels_us=%lld "
                    "down_us=%lld\n", n_in, chunk_no, mat_el * 8 + L.side_bytes(), launches, max_n, stage_us, (long long)(ms[0] * 1e3f),
                    (long long)(ms[1] * 1e3f), (long long)(ms[2] * 1e3f));
        }
        ++chunk_no;
        p0 = p1;
    }
    return IMPOP_OK;
}
