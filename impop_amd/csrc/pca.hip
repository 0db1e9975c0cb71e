// pca.hip — impop_pca_scan: its kernels, its PairEpilogue (pair_front.h) and the entry point.  Per window the k largest eigenpairs
// of the double-centred distance matrix B = -1/2 J H J of the members, by block subspace iteration with Rayleigh-Ritz (all
// arithmetic: pca_math.h), and once per call the window-to-window distances from the vectors of all windows.
//
// Eigen kernel: one workgroup per window, of 256 threads up to 256 members, 512 up to 512, 1024 beyond, so that a thread owns
// one row of the block (the template keeps R rows per thread; only R = 1 is built: two rows spilt far more registers than the
// wider workgroup does).  B is never formed.  The workgroup first gathers the symmetric m x m distance matrix H (uint16 where every distance fits, else uint32) into its slice of the epilogue's scratch, from the Gram
// kernel's upper triangle: the one strided pass; every iteration then reads H unit-stride out of L2.  The block V (m x 16
// doubles, column-major) sits in LDS; a thread holds its row of the product block in registers.
// H V is plain VALU fma — per member j one coalesced load of H[j][row] per owned row, 16 broadcast LDS reads of V[j][:] — and
// -1/2 J (H V) = B V because V is kept orthogonal to the ones vector.  Everything else an iteration does is local to a row except
// the sums over rows, which all go through one reduction: a transposing fold of 16 values per lane inside a wave, the waves
// added in order (fixed order, no atomics).  The 16 x 16 Jacobi runs on 256 threads, one matrix element each.
#include "pair_front.h"
#include "pca_math.h"

namespace impop {

constexpr int PCA_T = 256;  // threads of the distance kernel

// The eigen kernel: one workgroup per Gram problem; the members are positions 0 .. m - 1 in ascending haplotype index.  The distance
// kernel: once per call, over the vectors of all windows in the caller's window order.
struct PcaIn {
    const uint32_t *hap_of;  // m: haplotype index of a position
    void *hs;                // scratch: n_problems x m x m distances, symmetric, uint16 where h16 else uint32
    const uint64_t *ord;     // problem p is window ord[p] of the call (the slot of the all-window tables), or nullptr
    uint32_t m, k, max_iter, h16;
    double tol;
};
struct PcaOut {
    impop_pca_window *rec;   // n_problems
    double *vec;             // n_problems x k x m, or nullptr
    double *all_vec;         // per WINDOW of the call: k x m | 8 eigenvalues | usable by the distance kernel; or nullptr
    double *all_lam;
    uint32_t *all_ok;
};

// ---- the one reduction: every thread brings 16 partial sums; afterwards the workgroup's 16 totals are pca_tot(red, buf, q)
template <int HALF, int BIT>
__device__ __forceinline__ void pca_fold_stage(double (&v)[PCA_B], uint32_t lane) {
    const bool up = (lane & BIT) != 0;
#pragma unroll
    for (int i = 0; i < HALF; ++i) {
        const double send = up ? v[i] : v[i + HALF], keep = up ? v[i + HALF] : v[i];
        v[i] = keep + __shfl_xor(send, BIT, 64);
    }
}
// red: [2][16 waves][16]; two buffers in turn, so that one barrier per reduction is enough
constexpr int PCA_RED = 16 * PCA_B;  // doubles per buffer
__device__ __forceinline__ void pca_reduce16(double (&p)[PCA_B], double *red, int &buf) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    pca_fold_stage<8, 32>(p, lane);
    pca_fold_stage<4, 16>(p, lane);
    pca_fold_stage<2, 8>(p, lane);
    pca_fold_stage<1, 4>(p, lane);
    double v = p[0];
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 1, 64);  // lane 4 q holds the wave's sum of value q
    buf ^= 1;
    if ((lane & 3u) == 0) red[buf * PCA_RED + wave * PCA_B + (lane >> 2)] = v;
    __syncthreads();
}
template <int NW>  // the waves in order
__device__ __forceinline__ double pca_tot(const double *red, int buf, int q) {
    const double *r = red + buf * PCA_RED + q;
    double s = r[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) s += r[w * PCA_B];
    return s;
}

struct PcaLds {
    double *V, *G, *Q, *red, *cs, *ts, *theta, *resid, *tmp;
    uint64_t *sh;
    uint32_t *hap, *diag;
    int *order, *ctl;  // ctl: 0 sweep flag, 1 rank, 2 done
};
__host__ __device__ inline size_t pca_lds_doubles(uint32_t m) { return (size_t)PCA_B * m + 4 * 256 + 2 * 16 * PCA_B + 5 * PCA_B + 16; }
__device__ __forceinline__ PcaLds pca_carve(double *base, uint32_t m) {
    PcaLds L;
    L.V = base; L.G = L.V + (size_t)PCA_B * m; L.Q = L.G + 512; L.red = L.Q + 512;
    L.cs = L.red + 2 * PCA_RED; L.ts = L.cs + PCA_B; L.theta = L.ts + PCA_B; L.resid = L.theta + PCA_B; L.tmp = L.resid + PCA_B;
    L.sh = reinterpret_cast<uint64_t *>(L.tmp + PCA_B);  // 16 words
    L.hap = reinterpret_cast<uint32_t *>(L.sh + 16);
    L.diag = L.hap + m;
    L.order = reinterpret_cast<int *>(L.diag + m);
    L.ctl = L.order + PCA_B;
    return L;
}
static size_t pca_eigen_lds_bytes(uint32_t m) { return pca_lds_doubles(m) * 8 + (size_t)m * 8 + (PCA_B + 8) * 4; }

// orthonormalise the block held in the threads' rows (inactive rows are zero) and leave it in LDS
template <int NT, int R>
__device__ __forceinline__ void pca_orthonormalise(double (&z)[R][PCA_B], const PcaLds &L, int &buf, uint32_t m) {
    const uint32_t tid = threadIdx.x;
    {
        double p[PCA_B];
#pragma unroll
        for (int c = 0; c < PCA_B; ++c) {
            p[c] = 0.0;
#pragma unroll
            for (int t = 0; t < R; ++t) p[c] += z[t][c];
        }
        pca_reduce16(p, L.red, buf);
        double mean[PCA_B];
#pragma unroll
        for (int c = 0; c < PCA_B; ++c) mean[c] = pca_mean(pca_tot<NT / 64>(L.red, buf, c), m);
#pragma unroll
        for (int t = 0; t < R; ++t)
            if (tid + NT * t < m) pca_centre_row(z[t], mean);
    }
#pragma unroll
    for (int j = 0; j < PCA_B; ++j) {
        double n0 = 0.0;
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            double p[PCA_B];
#pragma unroll
            for (int c = 0; c < PCA_B; ++c) p[c] = 0.0;
#pragma unroll
            for (int t = 0; t < R; ++t) pca_gs_partials(z[t], j, p);
            pca_reduce16(p, L.red, buf);
            double dots[PCA_B];
#pragma unroll
            for (int i = 0; i <= j; ++i) dots[i] = pca_tot<NT / 64>(L.red, buf, i);
            if (pass == 0) n0 = dots[j];
#pragma unroll
            for (int t = 0; t < R; ++t) pca_gs_subtract(z[t], j, dots);
        }
        double p[PCA_B];
#pragma unroll
        for (int c = 0; c < PCA_B; ++c) p[c] = 0.0;
#pragma unroll
        for (int t = 0; t < R; ++t) p[0] += pca_sq(z[t][j]);
        pca_reduce16(p, L.red, buf);
        const double s = pca_gs_scale(n0, pca_tot<NT / 64>(L.red, buf, 0));
#pragma unroll
        for (int t = 0; t < R; ++t) z[t][j] *= s;
    }
#pragma unroll
    for (int t = 0; t < R; ++t)
        if (tid + NT * t < m) {
#pragma unroll
            for (int c = 0; c < PCA_B; ++c) L.V[(size_t)c * m + tid + NT * t] = z[t][c];
        }
    __syncthreads();
}

template <typename HT, int NT, int R>
__global__ __launch_bounds__(NT) void pca_eigen_kernel(SimBatch batch, const impop_window_stats *__restrict__ ws, PcaIn in, PcaOut out) {
    extern __shared__ double pca_smem[];
    const uint32_t m = in.m, k = in.k, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t w = blockIdx.x;
    const PcaLds L = pca_carve(pca_smem, m);
    const SimView S = sim_view(batch, w);
    const bool no_sites = S.W == 0;  // every H is 0
    const uint32_t cols = pca_block_cols(m);
    const double nan = __builtin_nan("");
    int buf = 0;

    // ---- gather: H symmetric into scratch, from the Gram upper triangle (members ascend, so (p, q > p) is (min, max)); sum_h
    for (uint32_t p = tid; p < m; p += NT) {
        const uint32_t h = in.hap_of[p];
        L.hap[p] = h;
        L.diag[p] = no_sites ? 0u : (uint32_t)gram_at(S, h, h);
    }
    __syncthreads();
    HT *Hs = reinterpret_cast<HT *>(in.hs) + w * (uint64_t)m * m;
    uint64_t part = 0;
    for (uint32_t p = wave; p < m; p += NT / 64) {
        const uint32_t hp = L.hap[p], ap = L.diag[p];
        for (uint32_t q = p + lane; q < m; q += 64) {
            uint32_t H = 0;
            if (q != p && !no_sites) H = ap + L.diag[q] - 2u * (uint32_t)gram_at(S, hp, L.hap[q]);
            Hs[(uint64_t)p * m + q] = (HT)H;
            Hs[(uint64_t)q * m + p] = (HT)H;
            part += H;
        }
    }
    const uint64_t sum_h = block_sum_u64_n<NT>(part, L.sh);
    __threadfence_block();  // H was written by other waves of this workgroup
    __syncthreads();

    uint32_t iterations = 0, flags = 0;
    const uint64_t slot = in.ord ? in.ord[w] : w;
    double *vec = out.vec ? out.vec + w * (uint64_t)k * m : nullptr;
    double *avec = out.all_vec ? out.all_vec + slot * (uint64_t)k * m : nullptr;

    uint32_t rank = 0;
    double z[R][PCA_B];
    if (sum_h != 0) {
        const double trace = pca_trace(sum_h, m);
#pragma unroll
        for (int t = 0; t < R; ++t)
#pragma unroll
            for (int c = 0; c < PCA_B; ++c) z[t][c] = tid + NT * t < m ? pca_start(tid + NT * t, (uint32_t)c, cols) : 0.0;
        pca_orthonormalise<NT, R>(z, L, buf, m);
        double *A = L.G, *An = L.G + 256, *Q = L.Q, *Qn = L.Q + 256;
        const bool el = tid < 256u;  // the threads that own an element of the 16 x 16 matrices
        const int ei = (int)((tid >> 4) & 15u), ej = (int)(tid & 15u);
        for (uint32_t it = 1;; ++it) {
            // ---- Z = -1/2 J (H V)
#pragma unroll
            for (int t = 0; t < R; ++t)
#pragma unroll
                for (int c = 0; c < PCA_B; ++c) z[t][c] = 0.0;
            for (uint32_t j = 0; j < m; ++j) {
                const HT *hrow = Hs + (uint64_t)j * m;
                double h[R];
#pragma unroll
                for (int t = 0; t < R; ++t) h[t] = tid + NT * t < m ? (double)hrow[tid + NT * t] : 0.0;
#pragma unroll
                for (int t = 0; t < R; ++t)
                    if (wave * 64 + NT * t < m) pca_hv_add(z[t], h[t], L.V + j, m);  // a wave without rows skips
            }
            {
                double p[PCA_B];
#pragma unroll
                for (int c = 0; c < PCA_B; ++c) {
                    p[c] = 0.0;
#pragma unroll
                    for (int t = 0; t < R; ++t) p[c] += z[t][c];
                }
                pca_reduce16(p, L.red, buf);
                double mean[PCA_B];
#pragma unroll
                for (int c = 0; c < PCA_B; ++c) mean[c] = pca_mean(pca_tot<NT / 64>(L.red, buf, c), m);
#pragma unroll
                for (int t = 0; t < R; ++t)
                    if (tid + NT * t < m) pca_bv_row(z[t], mean);
            }
            // ---- G = V^T Z, row i from one reduction; the upper triangle mirrored
            for (int i = 0; i < PCA_B; ++i) {
                double p[PCA_B];
#pragma unroll
                for (int c = 0; c < PCA_B; ++c) p[c] = 0.0;
#pragma unroll
                for (int t = 0; t < R; ++t) pca_dot_partials(tid + NT * t < m ? L.V[(size_t)i * m + tid + NT * t] : 0.0, z[t], p);
                pca_reduce16(p, L.red, buf);
                if ((int)tid >= i && tid < (uint32_t)PCA_B) {
                    const double g = pca_tot<NT / 64>(L.red, buf, (int)tid);
                    A[i * PCA_B + tid] = g;
                    A[tid * PCA_B + i] = g;
                }
            }
            if (el) Q[tid] = ei == ej ? 1.0 : 0.0;
            __syncthreads();
            // ---- Jacobi: thread (ei, ej) owns one element of A and of Q
            const double thr = pca_jacobi_threshold(A);
            for (int sweep = 0; sweep < PCA_MAX_SWEEPS; ++sweep) {
                if (tid == 0) L.ctl[0] = 0;
                __syncthreads();
                if (el && ei < ej && fabs(A[tid]) > thr) L.ctl[0] = 1;
                __syncthreads();
                if (!L.ctl[0]) break;
                for (int round = 0; round < 15; ++round) {
                    if (tid < (uint32_t)PCA_B) pca_jacobi_round_angles(A, thr, round, (int)tid, L.cs, L.ts);
                    __syncthreads();
                    if (el) {
                        An[tid] = pca_jacobi_elem(A, L.cs, L.ts, round, ei, ej);
                        Qn[tid] = pca_jacobi_qelem(Q, L.cs, L.ts, round, ei, ej);
                    }
                    __syncthreads();
                    double *s = A; A = An; An = s;
                    s = Q; Q = Qn; Qn = s;
                }
            }
            if (tid == 0) {
                pca_sort_desc(A, cols, L.order);
                for (int c = 0; c < PCA_B; ++c) L.theta[c] = A[L.order[c] * PCA_B + L.order[c]];
            }
            __syncthreads();
            if (el) Qn[tid] = Q[ei * PCA_B + L.order[ej]];  // the columns of Q in the order of theta
            __syncthreads();
            // ---- Ritz vectors X = V Qs, B X = Z Qs, residuals
            {
                double p[PCA_B];
#pragma unroll
                for (int c = 0; c < PCA_B; ++c) p[c] = 0.0;
#pragma unroll
                for (int t = 0; t < R; ++t)
                    if (wave * 64 + NT * t < m) {
                        const bool live = tid + NT * t < m;
                        {
                            double zq[PCA_B];
                            pca_rotate_row(z[t], Qn, zq);
#pragma unroll
                            for (int c = 0; c < PCA_B; ++c) z[t][c] = zq[c];
                        }
                        double v[PCA_B], x[PCA_B];
#pragma unroll
                        for (int c = 0; c < PCA_B; ++c) v[c] = live ? L.V[(size_t)c * m + tid + NT * t] : 0.0;
                        pca_rotate_row(v, Qn, x);
                        pca_resid_partials(z[t], x, L.theta, p);
                    }
                pca_reduce16(p, L.red, buf);
                if (tid < (uint32_t)PCA_B) L.resid[tid] = sqrt(pca_tot<NT / 64>(L.red, buf, (int)tid));
                __syncthreads();
                if (tid == 0) {
                    const uint32_t r = pca_rank(L.theta, k, cols, in.tol, trace);
                    const bool ok = pca_converged(L.resid, L.theta, r, in.tol);
                    L.ctl[1] = (int)r;
                    L.ctl[2] = ok ? 1 : (it >= in.max_iter ? 2 : 0);
                }
                __syncthreads();
            }
            if (L.ctl[2]) {
                iterations = it;
                flags = L.ctl[2] == 1 ? 0u : PCA_FLAG_UNCONVERGED;
                break;
            }
            pca_orthonormalise<NT, R>(z, L, buf, m);
            // (Qn is read by nobody any more; A, An, Q are rewritten by the next step behind barriers)
        }
        rank = (uint32_t)L.ctl[1];
        // ---- the vectors: X = V Qs once more (Qn still holds Qs), centred, unit length, the sign rule
        {
            double p[PCA_B];
#pragma unroll
            for (int c = 0; c < PCA_B; ++c) p[c] = 0.0;
#pragma unroll
            for (int t = 0; t < R; ++t) {
                const bool live = tid + NT * t < m;
                double v[PCA_B];
#pragma unroll
                for (int c = 0; c < PCA_B; ++c) v[c] = live ? L.V[(size_t)c * m + tid + NT * t] : 0.0;
                pca_rotate_row(v, Qn, z[t]);
#pragma unroll
                for (int c = 0; c < PCA_B; ++c) p[c] += z[t][c];
            }
            pca_reduce16(p, L.red, buf);
            double mean[PCA_B];
#pragma unroll
            for (int c = 0; c < PCA_B; ++c) { mean[c] = pca_mean(pca_tot<NT / 64>(L.red, buf, c), m); p[c] = 0.0; }
#pragma unroll
            for (int t = 0; t < R; ++t) {
                if (tid + NT * t < m) pca_centre_row(z[t], mean);
#pragma unroll
                for (int c = 0; c < PCA_B; ++c) p[c] += pca_sq(z[t][c]);
            }
            pca_reduce16(p, L.red, buf);
#pragma unroll
            for (int c = 0; c < PCA_B; ++c) {
                const double n = pca_tot<NT / 64>(L.red, buf, c), s = n > 0.0 ? 1.0 / sqrt(n) : 0.0;
#pragma unroll
                for (int t = 0; t < R; ++t)
                    if (tid + NT * t < m) L.V[(size_t)c * m + tid + NT * t] = z[t][c] * s;
            }
            __syncthreads();
            if (tid < rank) L.tmp[tid] = L.V[(size_t)tid * m + pca_sign_pivot(L.V + (size_t)tid * m, m)] < 0.0 ? -1.0 : 1.0;
            __syncthreads();
        }
    }
    for (uint32_t j = 0; j < k; ++j)
        for (uint32_t r = tid; r < m; r += NT) {
            const double v = j < rank ? L.tmp[j] * L.V[(size_t)j * m + r] : 0.0;
            if (vec) vec[(uint64_t)j * m + r] = v;
            if (avec) avec[(uint64_t)j * m + r] = v;
        }
    if (tid == 0) {
        impop_pca_window *rec = out.rec + w;
        rec->n_members = m; rec->n_sites = ws[w].n_sites; rec->rank = rank; rec->iterations = iterations; rec->flags = flags;
        rec->reserved = 0; rec->sum_h = sum_h;
        for (uint32_t j = 0; j < PCA_MAX_K; ++j) {
            const double lam = j < rank ? L.theta[j] : j < k ? 0.0 : nan;
            rec->lambda[j] = lam;
            rec->resid[j] = j < rank ? L.resid[j] : nan;
            if (avec) out.all_lam[slot * PCA_MAX_K + j] = lam;  // the three all-window tables come together
        }
        if (avec) out.all_ok[slot] = (rank > 0 && flags == 0) ? 1u : 0u;
    }
}

// ---- window-to-window distances.  One workgroup per window a, its vectors in LDS; a wave per later window b: the K x K dot
// products over the members (lanes stride the members, one butterfly per product), then pca_dist2, written to (a, b) and (b, a).
template <int K>
__global__ __launch_bounds__(PCA_T) void pca_dist_kernel(const double *__restrict__ vec, const double *__restrict__ lam,
                                                         const uint32_t *__restrict__ ok, uint32_t m, uint64_t n, double *__restrict__ out) {
    extern __shared__ double pca_smem[];
    const uint64_t a = blockIdx.x;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const double nan = __builtin_nan("");
    const bool ok_a = ok[a] != 0;
    if (tid == 0) out[a * n + a] = ok_a ? 0.0 : nan;
    if (!ok_a) {
        for (uint64_t b = a + 1 + tid; b < n; b += PCA_T) { out[a * n + b] = nan; out[b * n + a] = nan; }
        return;
    }
    const double *va = vec + a * (uint64_t)K * m;
    for (uint32_t i = tid; i < (uint32_t)K * m; i += PCA_T) pca_smem[i] = va[i];
    __syncthreads();
    for (uint64_t b = a + 1 + wave; b < n; b += PCA_T / 64) {
        if (!ok[b]) {
            if (lane == 0) { out[a * n + b] = nan; out[b * n + a] = nan; }
            continue;
        }
        const double *vb = vec + b * (uint64_t)K * m;
        double acc[K * K];
#pragma unroll
        for (int i = 0; i < K * K; ++i) acc[i] = 0.0;
        for (uint32_t r = lane; r < m; r += 64) {
            double y[K];
#pragma unroll
            for (int l = 0; l < K; ++l) y[l] = vb[(uint64_t)l * m + r];
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const double x = pca_smem[(size_t)j * m + r];
#pragma unroll
                for (int l = 0; l < K; ++l) acc[j * K + l] = fma(x, y[l], acc[j * K + l]);
            }
        }
#pragma unroll
        for (int i = 0; i < K * K; ++i) acc[i] = wave_sum_f64(acc[i]);
        if (lane == 0) {
            const double d = pca_dist2(K, lam + a * PCA_MAX_K, lam + b * PCA_MAX_K, acc);
            out[a * n + b] = d;
            out[b * n + a] = d;
        }
    }
}

template <typename HT, int NT, int R>
static int launch_eigen_as(impop_ctx *ctx, const SimBatch &b, uint64_t n, const impop_window_stats *d_stats, const PcaIn &in, const PcaOut &out,
                           size_t lds) {
    const int rc = lds_opt_in(pca_eigen_kernel<HT, NT, R>, lds);
    if (rc) return rc;
    hipLaunchKernelGGL((pca_eigen_kernel<HT, NT, R>), dim3((uint32_t)n), dim3(NT), lds, ctx->stream, b, d_stats, in, out);
    return IMPOP_OK;
}

static int launch_pca_eigen(impop_ctx *ctx, const SimBatch &b, uint64_t n_problems, const impop_window_stats *d_stats, const PcaIn &in,
                     const PcaOut &out) {
    if (!n_problems) return IMPOP_OK;
    REQUIRE(in.m >= 2 && in.m <= PCA_MAX_N && in.k >= 1 && in.k <= PCA_MAX_K && in.max_iter >= 1, "launch_pca_eigen: bad shape");
    const size_t lds = pca_eigen_lds_bytes(in.m);
    REQUIRE(lds <= 160 * 1024, "launch_pca_eigen: %zu bytes of LDS", lds);
    int rc;
    if (in.h16) rc = in.m <= 256 ? launch_eigen_as<uint16_t, 256, 1>(ctx, b, n_problems, d_stats, in, out, lds)
                   : in.m <= 512 ? launch_eigen_as<uint16_t, 512, 1>(ctx, b, n_problems, d_stats, in, out, lds)
                                 : launch_eigen_as<uint16_t, 1024, 1>(ctx, b, n_problems, d_stats, in, out, lds);
    else rc = in.m <= 256 ? launch_eigen_as<uint32_t, 256, 1>(ctx, b, n_problems, d_stats, in, out, lds)
            : in.m <= 512 ? launch_eigen_as<uint32_t, 512, 1>(ctx, b, n_problems, d_stats, in, out, lds)
                          : launch_eigen_as<uint32_t, 1024, 1>(ctx, b, n_problems, d_stats, in, out, lds);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return IMPOP_OK;
}

template <int K>
static int launch_dist_as(impop_ctx *ctx, const double *d_vec, const double *d_lam, const uint32_t *d_ok, uint32_t m, uint64_t n, double *d_out) {
    const size_t lds = (size_t)K * m * 8;
    const int rc = lds_opt_in(pca_dist_kernel<K>, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(pca_dist_kernel<K>, dim3((uint32_t)n), dim3(PCA_T), lds, ctx->stream, d_vec, d_lam, d_ok, m, n, d_out);
    return IMPOP_OK;
}

static int launch_pca_dist(impop_ctx *ctx, const double *d_vec, const double *d_lam, const uint32_t *d_ok, uint32_t m, uint32_t k,
                    uint64_t n_windows, double *d_out) {
    if (!n_windows) return IMPOP_OK;
    REQUIRE(m >= 2 && m <= PCA_MAX_N && k >= 1 && k <= PCA_MAX_K, "launch_pca_dist: bad shape");
    int rc = IMPOP_OK;
    switch (k) {
        case 1: rc = launch_dist_as<1>(ctx, d_vec, d_lam, d_ok, m, n_windows, d_out); break;
        case 2: rc = launch_dist_as<2>(ctx, d_vec, d_lam, d_ok, m, n_windows, d_out); break;
        case 3: rc = launch_dist_as<3>(ctx, d_vec, d_lam, d_ok, m, n_windows, d_out); break;
        case 4: rc = launch_dist_as<4>(ctx, d_vec, d_lam, d_ok, m, n_windows, d_out); break;
        case 5: rc = launch_dist_as<5>(ctx, d_vec, d_lam, d_ok, m, n_windows, d_out); break;
        case 6: rc = launch_dist_as<6>(ctx, d_vec, d_lam, d_ok, m, n_windows, d_out); break;
        case 7: rc = launch_dist_as<7>(ctx, d_vec, d_lam, d_ok, m, n_windows, d_out); break;
        default: rc = launch_dist_as<8>(ctx, d_vec, d_lam, d_ok, m, n_windows, d_out); break;
    }
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return IMPOP_OK;
}

// impop_pca_scan's epilogue: one launch of the eigen kernel per chunk — records and vectors; the symmetric distance matrices the
// kernel gathers live in scratch, one per window of a chunk.  With the window distances wanted, every window's vectors, eigenvalues
// and usability also go to tables that live across the chunks, in the caller's window order.
struct PcaEpilogue final : PairEpilogue {
    uint32_t M, k, max_iter;
    double tol;
    bool h16, want_dist;
    uint64_t n_windows;
    const std::vector<uint32_t> *hap_of;
    Result<impop_pca_window> rec;
    Result<double> vec;
    uint64_t launches = 0;
    uint32_t *d_hap = nullptr, *d_ok = nullptr;
    char *d_hs = nullptr;
    uint64_t *d_ord = nullptr;
    double *d_allvec = nullptr, *d_lam = nullptr, *d_dist = nullptr;
    size_t hs_bytes() const { return (size_t)M * M * (h16 ? 2 : 4); }
    // the device bytes layout() takes per window of a chunk (they bound a chunk: impop_pca_scan)
    size_t per_window_bytes() const { return hs_bytes() + sizeof(impop_pca_window) + (size_t)k * M * 8 + 8; }
    void layout(Layout &D, Layout &H, uint64_t cap) override {
        D.sub(d_hap, M); D.sub(d_ord, cap); rec.layout(D, H, cap); vec.layout(D, H, cap);
        D.sub(d_allvec, want_dist ? n_windows * k * M : 0); D.sub(d_lam, want_dist ? n_windows * 8 : 0);
        D.sub(d_ok, want_dist ? n_windows : 0); D.sub(d_dist, want_dist ? n_windows * n_windows : 0);
        D.sub(d_hs, cap * hs_bytes());
    }
    int upload(impop_ctx *ctx) override {
        HIP_TRY(hipMemcpyAsync(d_hap, hap_of->data(), (size_t)M * 4, hipMemcpyHostToDevice, ctx->stream));
        return IMPOP_OK;
    }
    int launch(impop_ctx *ctx, const PairChunk &c) override {
        if (want_dist) HIP_TRY(hipMemcpyAsync(d_ord, c.ord, c.cnt * 8, hipMemcpyHostToDevice, ctx->stream));
        const PcaIn in{d_hap, d_hs, want_dist ? d_ord : nullptr, M, k, max_iter, h16 ? 1u : 0u, tol};
        const PcaOut O{rec.d, vec.n ? vec.d : nullptr, want_dist ? d_allvec : nullptr, want_dist ? d_lam : nullptr,
                       want_dist ? d_ok : nullptr};  // (a table of zero bytes shares its offset with what follows it)
        // the eigen kernel between two events of its own: impop_ctx_pca_elapsed
        int rc = timed(ctx, ctx->timers[impop_ctx::T_PCA], [&] { return launch_pca_eigen(ctx, c.b, c.cnt, c.d_s, in, O); });
        if (rc) return rc;
        ++launches;
        if ((rc = rec.down(ctx, c.cnt))) return rc;
        return vec.down(ctx, c.cnt);
    }
    void collect(const PairChunk &c) override { rec.scatter(c); vec.scatter(c); }
};

}  // namespace impop

using namespace impop;

static_assert(sizeof(impop_pca_params) == 24 && sizeof(impop_pca_window) == 160, "fixed record layouts");
static_assert(IMPOP_PCA_MAX_N == PCA_MAX_N && IMPOP_PCA_MAX_K == PCA_MAX_K && PCA_MAX_K + 8 <= PCA_B, "the block holds k + 8 columns");

IMPOP_API int impop_pca_scan(impop_ctx *ctx, const impop_matrix *m, const impop_window *windows, uint64_t n_windows,
                             const uint64_t *mask_p, const impop_pca_params *params, impop_pca_window *out_windows, double *out_vectors,
                             double *out_dist2) {
    const char *fn = "impop_pca_scan";
    REQUIRE(ctx && m && params, "%s: NULL argument", fn);
    REQUIRE(params->struct_size == sizeof(impop_pca_params), "impop_pca_params.struct_size mismatch");
    REQUIRE(params->k >= 1 && params->k <= IMPOP_PCA_MAX_K, "%s: k must be 1..%u", fn, (uint32_t)IMPOP_PCA_MAX_K);
    REQUIRE(params->tol >= 1e-13 && params->tol <= 1e-2, "%s: tol must be in [1e-13, 1e-2]", fn);
    REQUIRE(params->max_iter >= 1 && params->max_iter <= 100000, "%s: max_iter must be 1..100000", fn);
    const std::vector<uint32_t> hap_of = mask_members(mask_p, m->g.n_hap);
    REQUIRE(hap_of.size() >= 2, "%s: the mask holds %zu members, fewer than 2", fn, hap_of.size());
    if (hap_of.size() > IMPOP_PCA_MAX_N) {  // refused before anything is uploaded or launched
        set_error("%s: the mask holds %zu members, more than the limit of %u", fn, hap_of.size(), (uint32_t)IMPOP_PCA_MAX_N);
        return IMPOP_E_UNSUPPORTED;
    }
    if (out_dist2 && n_windows > 16384) {
        set_error("%s: window distances of %llu windows, more than the limit of 16384", fn, (unsigned long long)n_windows);
        return IMPOP_E_UNSUPPORTED;
    }
    REQUIRE(!out_dist2 || out_vectors, "%s: out_dist2 needs out_vectors", fn);
    bool go;
    int rc = windows_ready(ctx, m, windows, n_windows, out_windows, fn, &go);
    if (rc || !go) return rc;
    const uint64_t max_W = widest_W(m, windows, n_windows);
    PcaEpilogue epi;
    epi.M = (uint32_t)hap_of.size(); epi.k = params->k; epi.max_iter = params->max_iter; epi.tol = params->tol;
    epi.h16 = max_W < 65536;  // a distance is at most its window's W
    epi.want_dist = out_dist2 != nullptr; epi.n_windows = n_windows;
    epi.hap_of = &hap_of;
    epi.rec.want(out_windows, 1); epi.vec.want(out_vectors, (size_t)epi.k * epi.M);
    // the gathered distance matrices and the vectors of a chunk: at most 1 GiB of them
    PairFront in = hamming_front(fn, max_W, chunk_windows(1ull << 30, epi.per_window_bytes()));
    rc = pairwise_front(ctx, m, windows, n_windows, in, epi);
    if (rc) return rc;
    if (out_dist2) {  // the scratch the front end bound the all-window tables into is still the context's
        rc = timed(ctx, ctx->timers[impop_ctx::T_PCA + 1],
                   [&] { return launch_pca_dist(ctx, epi.d_allvec, epi.d_lam, epi.d_ok, epi.M, epi.k, n_windows, epi.d_dist); });
        if (rc) return rc;
        ++epi.launches;
        HIP_TRY(hipMemcpyAsync(out_dist2, epi.d_dist, n_windows * n_windows * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    if (trace_on()) {
        uint32_t it_max = 0;
        uint64_t bad = 0;
        for (uint64_t i = 0; i < n_windows; ++i) {
            it_max = std::max(it_max, out_windows[i].iterations);
            bad += out_windows[i].flags & 1u;
        }
        fprintf(stderr, "[impop_pca_scan] route=%s members=%u k=%u windows=%llu chunks=%llu launches=%llu iterations_max=%u unconverged=%llu "
                "dist=%s\n", m->compact ? "compact" : "dense", epi.M, epi.k, (unsigned long long)n_windows, (unsigned long long)in.chunks,
                (unsigned long long)epi.launches, it_max, (unsigned long long)bad, out_dist2 ? "on" : "off");
    }
    return IMPOP_OK;
}
