// ehh.hip — extended haplotype homozygosity on the resident bit matrix: the reference's
// calc_EHH (scripts/wip/ehhgfa.py:6-21, ehh2.py:76-89).
//
// EHH[i] = round(#{pairs j<k identical on the first i+1 sites} / (m(m-1)/2), 3).  A pair stays
// "homozygous" exactly until its first differing site f_jk, so the whole vector is the suffix count
// of the histogram of first-mismatch positions:
//     pairs(i) = C(m,2) - #{f_jk <= i}
//   1. ehh_transpose_kernel   SB64 window -> word-major [64-site block][haplotype] u64 (ballot
//                             transpose, window edges masked off), so that lane = haplotype reads
//                             are coalesced
//   2. ehh_first_diff_kernel  one thread per pair: XOR the two rows block by block until the first
//                             non-zero word; integer atomic into hist[f]
//   3. ehh_finalize_kernel    one workgroup: scan of hist, then the reference's division and
//                             CPython round(, 3) in fp64
//
// impop_ehh_scan keeps only the integral of each curve, for a batch of (window, core allele, half) problems:
//   1. ehh_scan_transpose_kernel  the ballot transpose with a window dimension (blockIdx.y), rows compacted to the
//                                 members of P, every window at its own base of the chunk scratch
//   2. ehh_refine_kernel          one workgroup per problem: partition refinement of the members (class label,
//                                 representative and size in LDS) along the walking direction; the curve only steps
//                                 where a class splits, so one lane integrates it as a run-length sum of thousandths
#include <string.h>

#include <algorithm>
#include <vector>

#include "chunk_run.h"
#include "device_utils.h"
#include "internal.h"
#include "win_chunks.h"

namespace impop {

__global__ __launch_bounds__(256) void ehh_transpose_kernel(const uint32_t *__restrict__ sb, uint32_t wps, uint32_t G, uint32_t r,
                                                            uint64_t site_begin, uint64_t site_end, uint32_t n_pad,
                                                            uint64_t *__restrict__ wm) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t blk0 = site_begin >> 6;
    const uint64_t bi = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint64_t b = blk0 + bi;
    if (b * 64 >= site_end) return;  // wave-uniform
    uint64_t edge = ~0ull;           // sites of this block inside [site_begin, site_end)
    if (b * 64 < site_begin) edge &= ~0ull << (site_begin - b * 64);
    if (site_end - b * 64 < 64) edge &= (1ull << (site_end - b * 64)) - 1ull;
    for (uint32_t k = 0; k < wps; ++k) {
        const uint64_t keep = ballot_transpose32(sb[sb_index(wps, G, r, b, lane, k)], lane);
        if (lane < 32) wm[bi * n_pad + 32 * k + lane] = keep & edge;
    }
}

// grid = (ceil(m/256), m): blockIdx.y = position a in the member list, threads = positions b > a
__global__ __launch_bounds__(256) void ehh_first_diff_kernel(const uint64_t *__restrict__ wm, uint32_t n_pad, uint64_t n_blk,
                                                             const uint32_t *__restrict__ idx, uint32_t m, uint64_t first_site_off,
                                                             uint64_t W, int reverse, unsigned long long *__restrict__ hist) {
    const uint32_t a = blockIdx.y;
    const uint32_t bpos = blockIdx.x * 256 + threadIdx.x;
    if (bpos <= a || bpos >= m) return;
    const uint32_t ra = idx[a], rb = idx[bpos];
    // bit position p of block t is window site t*64 + p - first_site_off
    if (!reverse) {
        for (uint64_t t = 0; t < n_blk; ++t) {
            const uint64_t x = wm[t * n_pad + ra] ^ wm[t * n_pad + rb];
            if (x) {
                const uint64_t f = t * 64 + (uint64_t)__builtin_ctzll(x) - first_site_off;
                atomicAdd(&hist[f], 1ull);
                return;
            }
        }
    } else {
        for (uint64_t t = n_blk; t-- > 0;) {
            const uint64_t x = wm[t * n_pad + ra] ^ wm[t * n_pad + rb];
            if (x) {
                const uint64_t pos = t * 64 + (63 - (uint64_t)__builtin_clzll(x)) - first_site_off;
                atomicAdd(&hist[W - 1 - pos], 1ull);
                return;
            }
        }
    }
}

constexpr int EHH_FT = 1024;
__global__ __launch_bounds__(EHH_FT) void ehh_finalize_kernel(const unsigned long long *__restrict__ hist, uint64_t W, uint32_t m,
                                                              double *__restrict__ out) {
    __shared__ unsigned long long part[EHH_FT];
    const uint32_t tid = threadIdx.x;
    const uint64_t per = (W + EHH_FT - 1) / EHH_FT;
    const uint64_t lo = (uint64_t)tid * per < W ? (uint64_t)tid * per : W;
    const uint64_t hi = lo + per < W ? lo + per : W;
    unsigned long long s = 0;
    for (uint64_t i = lo; i < hi; ++i) s += hist[i];
    part[tid] = s;
    __syncthreads();
    for (int off = 1; off < EHH_FT; off <<= 1) {  // inclusive Hillis-Steele scan over the chunk sums
        const unsigned long long v = tid >= (uint32_t)off ? part[tid - off] : 0ull;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    const unsigned long long total = (unsigned long long)m * (m - 1) / 2;
    const double denom = (double)((unsigned long long)m * (m - 1)) / 2.0;  // ehhgfa.py:20: m*(m-1)/2 (true division)
    unsigned long long broken = part[tid] - s;                            // pairs whose first difference is before lo
    for (uint64_t i = lo; i < hi; ++i) {
        broken += hist[i];
        out[i] = py_round((double)(total - broken) / denom, 3);
    }
}

__global__ void ehh_fill_kernel(double *out, uint64_t W, double v) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < W) out[i] = v;
}


// ---- impop_ehh_scan ------------------------------------------------------------------------------------------------
// one window of a chunk: its sites, and where its transposed words live (absolute 64-site blocks tblk0 .. tblk0 + n_blk)
struct EhhWin {
    uint64_t begin, end, core;
    uint64_t woff;   // first word of the window in the chunk scratch
    uint64_t tblk0;
    uint32_t n_blk, pad;
};

// grid = (ceil(max n_blk / 4), windows): wave = one 64-site block of window blockIdx.y; ppos[h] = position of haplotype h
// in P or -1 (padding rows included); row stride = |P|.  No edge masks: a problem masks its own range.
__global__ __launch_bounds__(256) void ehh_scan_transpose_kernel(const uint32_t *__restrict__ sb, uint32_t wps, uint32_t G, uint32_t r,
                                                                 const EhhWin *__restrict__ win, const int32_t *__restrict__ ppos,
                                                                 uint32_t stride, uint64_t *__restrict__ wm) {
    const EhhWin w = win[blockIdx.y];
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t bi = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (bi >= w.n_blk) return;  // wave-uniform
    const uint64_t b = w.tblk0 + bi;
    uint64_t *dst = wm + w.woff + bi * stride;
    for (uint32_t k = 0; k < wps; ++k) {
        const uint64_t keep = ballot_transpose32(sb[sb_index(wps, G, r, b, lane, k)], lane);
        if (lane < 32) {
            const int32_t pp = ppos[32 * k + lane];
            if (pp >= 0) dst[pp] = keep;
        }
    }
}

constexpr int EHH_ST = 256;          // threads of a refinement workgroup
constexpr int EHH_GRP = 4;           // 64-site blocks tested per barrier while nothing differs
constexpr uint32_t EHH_NONE = 0xFFFFFFFFu;
constexpr uint32_t EHH_NEWID = 0x80000000u;  // tmp[c] holds the id of the class split off c
constexpr uint16_t EHH_MOVER = 0x8000u, EHH_LEADER = 0x4000u, EHH_LABEL = 0x0FFFu;  // label bits (ids < 4096)
static_assert(IMPOP_EHH_SCAN_MAX_N <= EHH_LABEL + 1u, "class ids must fit the label bits");

__device__ inline long long ehh_milli(unsigned long long total, unsigned long long broken, double denom) {
    return llrint(1000.0 * py_round((double)(total - broken) / denom, 3));  // the double ehh_finalize_kernel writes, in thousandths
}

// workgroup minimum; slots alternate so that one barrier per call suffices
__device__ inline uint32_t ehh_block_min(uint32_t v, uint32_t (*slots)[EHH_ST / 64], uint32_t &par) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, off, 64));
    if ((threadIdx.x & 63) == 0) slots[par][threadIdx.x >> 6] = v;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < EHH_ST / 64; ++k) v = min(v, slots[par][k]);
    par ^= 1u;
    return v;
}

// grid = 4 problems per window: blockIdx.x = 4 * window + 2 * allele + half.  Dynamic LDS: 12 bytes x mcap (|P| rounded up
// to even): tmp u32 | size u16 | row u16 | label u16 | rep u16.
//   row[i]    position in P of member i (ascending)          label[i]  class of member i (+ the two step flags)
//   rep[c]    member that represents class c (never moves)   size[c]   members of class c (u16 halves of u32 atomics)
//   tmp[c]    during a step: smallest mover of c, then the id split off c; tmp[new id] = c; EHH_NONE between steps
__global__ __launch_bounds__(EHH_ST) void ehh_refine_kernel(const uint32_t *__restrict__ sb, uint32_t wps, uint32_t G, uint32_t r,
                                                            const EhhWin *__restrict__ win, const uint32_t *__restrict__ idx, uint32_t nP,
                                                            uint32_t mcap, int flanks, uint32_t ref_hap, const uint64_t *__restrict__ wm,
                                                            uint32_t stride, impop_ehh_stats *__restrict__ rec, uint32_t *__restrict__ err) {
    extern __shared__ uint32_t ehh_lds[];
    uint32_t *tmp = ehh_lds;
    uint32_t *size32 = tmp + mcap;
    uint16_t *size = reinterpret_cast<uint16_t *>(size32);
    uint16_t *row = size + mcap, *label = row + mcap, *rep = label + mcap;
    __shared__ uint32_t s_slots[2][EHH_ST / 64];
    __shared__ uint32_t s_ncls;
    __shared__ unsigned long long s_broken, s_chk;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t wi = blockIdx.x >> 2, a = (blockIdx.x >> 1) & 1u, half = blockIdx.x & 1u;
    const EhhWin w = win[wi];
    const uint64_t cb = w.core >> 6;
    const uint32_t cl = (uint32_t)(w.core & 63);

    // members of P carrying allele a at the core, in ascending order
    uint32_t m = 0;
    for (uint32_t base = 0; base < nP; base += EHH_ST) {
        const uint32_t j = base + tid;
        bool f = false;
        if (j < nP) {
            const uint32_t hp = idx[j];
            f = ((sb[sb_index(wps, G, r, cb, cl, hp >> 5)] >> (hp & 31)) & 1u) == a;
        }
        const uint64_t bal = __ballot(f);
        if (lane == 0) s_slots[0][wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t off = m, tot = 0;
#pragma unroll
        for (int k = 0; k < EHH_ST / 64; ++k) {
            if ((uint32_t)k < wave) off += s_slots[0][k];
            tot += s_slots[0][k];
        }
        if (f) row[off + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = (uint16_t)j;
        m += tot;
        __syncthreads();
    }

    // the half's sites [rb, re) and direction
    const bool reverse = half == 0;
    const bool right = half == 1 || flanks == IMPOP_EHH_FLANKS_REFERENCE;
    const uint64_t rb = right ? w.core + 1 : w.begin, re = right ? w.end : w.core;
    const uint64_t W = re - rb;
    if (tid == 0) {
        if (half == 0) {
            rec[wi].n_members[a] = m;
            rec[wi].area[a] = 0.0;  // the host fills it in from both halves
        }
        if ((blockIdx.x & 3u) == 0) {
            rec[wi].ref_allele = (sb[sb_index(wps, G, r, cb, cl, ref_hap >> 5)] >> (ref_hap & 31)) & 1u;
            rec[wi].reserved = 0;
        }
    }
    if (m < 2 || W == 0) {  // ehhgfa.py:17-18: one member -> 500 at every site; nobody, or no site -> 0
        if (tid == 0) rec[wi].area_milli[a][half] = (m == 1) ? (long long)(500000ull * W) : 0ll;
        return;
    }

    for (uint32_t i = tid; i < m; i += EHH_ST) {
        tmp[i] = EHH_NONE;
        size[i] = 0;
        label[i] = 0;
        rep[i] = 0;
    }
    if (tid == 0) {
        s_ncls = 1;
        s_broken = 0;
        s_chk = 0;
    }
    __syncthreads();
    if (tid == 0) size32[0] = m;  // size[0] = m (<= 4096), size[1] = 0
    __syncthreads();

    const unsigned long long total = (unsigned long long)m * (m - 1) / 2;
    const double denom = (double)((unsigned long long)m * (m - 1)) / 2.0;  // as ehh_finalize_kernel
    long long area = 0, k = ehh_milli(total, 0, denom);                    // thread 0's run-length sum
    uint64_t last = 0;                                                     // walking index up to which `area` is summed
    const uint64_t b_lo = rb >> 6, b_hi = (re - 1) >> 6, nb = b_hi - b_lo + 1;
    const uint64_t *wbase = wm + w.woff;
    uint32_t par = 1;
    bool done = false;
    for (uint64_t u = 0; u < nb && !done; u += EHH_GRP) {
        const uint32_t g = nb - u < (uint64_t)EHH_GRP ? (uint32_t)(nb - u) : (uint32_t)EHH_GRP;
        // the common case: no member differs from its representative anywhere in these blocks
        uint64_t acc = 0;
        for (uint32_t i = tid; i < m; i += EHH_ST) {
            const uint32_t ri = row[i], rr = row[rep[label[i]]];
            if (ri == rr) continue;
            for (uint32_t j = 0; j < g; ++j) {
                const uint64_t B = reverse ? b_hi - (u + j) : b_lo + (u + j);
                const uint64_t *p = wbase + (B - w.tblk0) * stride;
                uint64_t x = p[ri] ^ p[rr];
                if (B == b_lo) x &= ~0ull << (rb & 63);
                if (B == b_hi && (re & 63)) x &= (1ull << (re & 63)) - 1ull;
                acc |= x;
            }
        }
        if (!__syncthreads_or(acc != 0)) continue;
        for (uint32_t j = 0; j < g && !done; ++j) {
            const uint64_t B = reverse ? b_hi - (u + j) : b_lo + (u + j);
            const uint64_t *p = wbase + (B - w.tblk0) * stride;
            uint64_t mask = ~0ull;  // sites of the block inside the range and not yet walked
            if (B == b_lo) mask &= ~0ull << (rb & 63);
            if (B == b_hi && (re & 63)) mask &= (1ull << (re & 63)) - 1ull;
            while (mask) {
                // nearest differing site in walking direction
                uint32_t q = 64;
                for (uint32_t i = tid; i < m; i += EHH_ST) {
                    const uint32_t ri = row[i], rr = row[rep[label[i]]];
                    const uint64_t x = (p[ri] ^ p[rr]) & mask;
                    if (x) q = min(q, (uint32_t)(reverse ? __builtin_clzll(x) : __builtin_ctzll(x)));
                }
                q = ehh_block_min(q, s_slots, par);
                if (q == 64) break;
                const uint32_t sbit = reverse ? 63 - q : q;
                // movers: members that differ from their representative at this site; the smallest leads the new class
                for (uint32_t i = tid; i < m; i += EHH_ST) {
                    const uint32_t c = label[i];
                    const uint32_t ri = row[i], rr = row[rep[c]];
                    if (((p[ri] ^ p[rr]) >> sbit) & 1ull) {
                        label[i] = (uint16_t)(c | EHH_MOVER);
                        atomicMin(&tmp[c], i);
                    }
                }
                __syncthreads();
                for (uint32_t i = tid; i < m; i += EHH_ST) {
                    const uint32_t l = label[i];
                    if (!(l & EHH_MOVER)) continue;
                    const uint32_t c = l & EHH_LABEL;
                    if (tmp[c] == i) {  // other movers of c see the smallest mover or the flagged id, never their own index
                        const uint32_t id = atomicAdd(&s_ncls, 1u);
                        rep[id] = (uint16_t)i;
                        tmp[id] = c;
                        tmp[c] = EHH_NEWID | id;
                        label[i] = (uint16_t)(l | EHH_LEADER);
                    }
                }
                __syncthreads();
                for (uint32_t i = tid; i < m; i += EHH_ST) {
                    const uint32_t l = label[i];
                    if (!(l & EHH_MOVER)) continue;
                    const uint32_t c = l & EHH_LABEL, id = tmp[c] & ~EHH_NEWID;
                    atomicSub(&size32[c >> 1], (c & 1u) ? 0x10000u : 1u);
                    atomicAdd(&size32[id >> 1], (id & 1u) ? 0x10000u : 1u);
                    label[i] = (uint16_t)(id | (l & EHH_LEADER));
                }
                __syncthreads();
                unsigned long long br = 0;
                for (uint32_t i = tid; i < m; i += EHH_ST) {
                    const uint32_t l = label[i];
                    if (!(l & EHH_LEADER)) continue;
                    const uint32_t id = l & EHH_LABEL, c = tmp[id];
                    br += (unsigned long long)size[id] * size[c];  // pairs between the movers and those that stay
                    tmp[id] = EHH_NONE;
                    tmp[c] = EHH_NONE;
                    label[i] = (uint16_t)id;
                }
                if (br) atomicAdd(&s_broken, br);
                __syncthreads();
                const unsigned long long broken = s_broken;
                if (tid == 0) {
                    const uint64_t site = B * 64 + sbit, pos = reverse ? re - 1 - site : site - rb;
                    area += (long long)(pos - last) * k;
                    last = pos;
                    k = ehh_milli(total, broken, denom);
                }
                if (broken == total) {  // every class is a single member: the curve stays at its last value
                    done = true;
                    break;
                }
                mask &= reverse ? ((1ull << sbit) - 1ull) : (sbit == 63 ? 0ull : ~0ull << (sbit + 1));
            }
        }
    }
    // consistency: the classes that are left account for exactly the pairs that never broke
    unsigned long long chk = 0;
    const uint32_t ncls = s_ncls;
    for (uint32_t c = tid; c < ncls && c < m; c += EHH_ST) chk += (unsigned long long)size[c] * (size[c] - 1u) / 2;
    chk = wave_sum_u64(chk);
    if (lane == 0 && chk) atomicAdd(&s_chk, chk);
    __syncthreads();
    if (tid == 0) {
        area += (long long)(W - last) * k;
        rec[wi].area_milli[a][half] = area;
        if (s_chk != total - s_broken || ncls > m) atomicOr(err, DEV_ERR_EHH);
    }
}

}  // namespace impop

using namespace impop;

IMPOP_API int impop_ehh(impop_ctx *ctx, const impop_matrix *m, uint64_t site_begin, uint64_t site_end, const uint64_t *mask,
                        int reverse, double *ehh_out_host, uint32_t *n_members) {
    REQUIRE(ctx && m, "impop_ehh: NULL argument");
    NOT_COMPACT(m, "impop_ehh");
    REQUIRE(site_begin <= site_end && site_end <= m->g.n_site, "impop_ehh: bad site range");
    HIP_TRY(hipSetDevice(ctx->device));
    const std::vector<uint32_t> idx = member_set(mask, m->g.n_hap, m->g.wps).idx;
    const uint32_t mm = (uint32_t)idx.size();
    if (n_members) *n_members = mm;
    const uint64_t W = site_end - site_begin;
    if (!W) return IMPOP_OK;  // calc_EHH returns an empty vector
    REQUIRE(ehh_out_host, "impop_ehh: out is NULL");
    REQUIRE(mm <= 65535, "impop_ehh: more than 65535 member haplotypes not supported");
    const uint64_t blk0 = site_begin >> 6, n_blk = ((site_end + 63) >> 6) - blk0;
    const uint32_t n_pad = m->g.wps * 32;
    const size_t wm_bytes = (size_t)n_blk * n_pad * 8;
    REQUIRE(wm_bytes <= (64ull << 30), "impop_ehh: window too large (%llu MiB of transposed scratch)",
            (unsigned long long)(wm_bytes >> 20));
    Carve L;
    const size_t o_wm = L.take_bytes(wm_bytes), o_hist = L.take<unsigned long long>(W), o_out = L.take<double>(W),
                 o_idx = L.take<uint32_t>(mm ? mm : 1);
    void *d = nullptr;
    int rc = ctx_scratch(ctx, L.total(), &d);
    if (rc) return rc;
    uint64_t *d_wm = L.at<uint64_t>(d, o_wm);
    unsigned long long *d_hist = L.at<unsigned long long>(d, o_hist);
    double *d_out = L.at<double>(d, o_out);
    uint32_t *d_idx = L.at<uint32_t>(d, o_idx);
    if (mm < 2) {  // ehhgfa.py:17-18: fewer than two haplotypes -> every entry 500
        hipLaunchKernelGGL(ehh_fill_kernel, dim3((uint32_t)((W + 255) / 256)), dim3(256), 0, ctx->stream, d_out, W, 500.0);
    } else {
        REQUIRE((n_blk + 3) / 4 < 0x7FFFFFFFull, "impop_ehh: range too long");
        HIP_TRY(hipMemcpyAsync(d_idx, idx.data(), (size_t)mm * 4, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemsetAsync(d_hist, 0, W * 8, ctx->stream));
        hipLaunchKernelGGL(ehh_transpose_kernel, dim3((uint32_t)((n_blk + 3) / 4)), dim3(256), 0, ctx->stream, m->d_sb, m->g.wps,
                           m->g.G, m->g.r, site_begin, site_end, n_pad, d_wm);
        hipLaunchKernelGGL(ehh_first_diff_kernel, dim3((mm + 255) / 256, mm), dim3(256), 0, ctx->stream, d_wm, n_pad, n_blk, d_idx,
                           mm, site_begin - blk0 * 64, W, reverse ? 1 : 0, d_hist);
        hipLaunchKernelGGL(ehh_finalize_kernel, dim3(1), dim3(EHH_FT), 0, ctx->stream, d_hist, W, mm, d_out);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(ehh_out_host, d_out, W * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return IMPOP_OK;
}

IMPOP_API int impop_ehh_scan(impop_ctx *ctx, const impop_matrix *m, const impop_ehh_window *windows, uint64_t n_windows,
                             const uint64_t *mask_p, const impop_ehh_params *params, impop_ehh_stats *out_host) {
    static_assert(sizeof(impop_ehh_stats) == 64 && sizeof(impop_ehh_window) == 24 && sizeof(impop_ehh_params) == 24, "ABI layout");
    REQUIRE(ctx && m && params, "impop_ehh_scan: NULL argument");
    REQUIRE(params->struct_size == sizeof(impop_ehh_params), "impop_ehh_params.struct_size mismatch");
    NOT_COMPACT(m, "impop_ehh_scan");
    REQUIRE(params->flanks == IMPOP_EHH_FLANKS_REFERENCE || params->flanks == IMPOP_EHH_FLANKS_TWO_SIDED,
            "impop_ehh_scan: unknown flanks mode %d", params->flanks);
    const uint32_t n = m->g.n_hap, n_pad = m->g.wps * 32;
    REQUIRE(params->ref_hap < n, "impop_ehh_scan: ref_hap %u is not one of the %u haplotypes", params->ref_hap, n);
    const MemberSet P = member_set(mask_p, n, m->g.wps);
    const uint32_t nP = P.size();
    if (nP > IMPOP_EHH_SCAN_MAX_N) {
        set_error("impop_ehh_scan: %u members exceed the LDS-resident refinement limit (%u); impop_ehh takes one window of up to 65535",
                  nP, (uint32_t)IMPOP_EHH_SCAN_MAX_N);
        return IMPOP_E_UNSUPPORTED;
    }
    if (!n_windows) return IMPOP_OK;
    REQUIRE(windows && out_host, "impop_ehh_scan: NULL windows/out");
    for (uint64_t i = 0; i < n_windows; ++i)
        REQUIRE(windows[i].site_begin <= windows[i].core_site && windows[i].core_site < windows[i].site_end &&
                    windows[i].site_end <= m->g.n_site,
                "impop_ehh_scan: window %llu: bad range [%llu,%llu) or core %llu for %llu sites", (unsigned long long)i,
                (unsigned long long)windows[i].site_begin, (unsigned long long)windows[i].site_end,
                (unsigned long long)windows[i].core_site, (unsigned long long)m->g.n_site);
    HIP_TRY(hipSetDevice(ctx->device));

    // the windows' transposed blocks and the chunks they fall into (by scratch bytes; blockIdx.y holds 65535 windows)
    const uint32_t stride = nP ? nP : 1;
    const bool after_core = params->flanks == IMPOP_EHH_FLANKS_REFERENCE;  // the transposed range starts behind the core
    std::vector<uint32_t> nblk(n_windows);
    for (uint64_t i = 0; i < n_windows; ++i) {
        const uint64_t tb = after_core ? windows[i].core_site + 1 : windows[i].site_begin, te = windows[i].site_end;
        const uint64_t nb = (nP && te > tb) ? ((te + 63) >> 6) - (tb >> 6) : 0;
        REQUIRE(nb < 0x7FFFFFFFull, "impop_ehh_scan: window %llu too long", (unsigned long long)i);
        nblk[i] = (uint32_t)nb;
    }
    const std::vector<WinChunk> chunks = cut_windows(n_windows, chunk_budget(params->max_chunk_bytes), 65535,
                                                     [&](size_t, uint64_t i) { return (uint64_t)nblk[i] * stride * 8; });
    const size_t max_cnt = max_over(chunks, [](const WinChunk &c) { return c.w_end - c.w_begin; }),
                 max_words = max_over(chunks, [&](const WinChunk &c) {
                     uint64_t words = 0;
                     for (uint64_t i = c.w_begin; i < c.w_end; ++i) words += (uint64_t)nblk[i] * stride;
                     return words;
                 }, 0);
    REQUIRE(max_words * 8 <= (64ull << 30), "impop_ehh_scan: a window needs %llu MiB of transposed scratch",
            (unsigned long long)(max_words >> 17));

    // device: idx | ppos | chunk windows | chunk records | transposed words; the first four mirrored in page-locked staging
    Carve L;
    const size_t o_idx = L.take<uint32_t>(stride), o_ppos = L.take<int32_t>(n_pad), o_win = L.take<EhhWin>(max_cnt),
                 o_rec = L.take<impop_ehh_stats>(max_cnt), staged = L.total(), o_wm = L.take<uint64_t>(max_words);
    void *d = nullptr, *pin = nullptr;
    int rc = ctx_scratch(ctx, L.total(), &d);
    if (rc) return rc;
    rc = ctx_pinned(ctx, staged, &pin);
    if (rc) return rc;
    const ChunkRun run{ctx, "impop_ehh_scan", (char *)d, (char *)pin};
    char *dc = run.dc, *hc = run.hc;
    if (nP) memcpy(hc + o_idx, P.idx.data(), (size_t)nP * 4);
    memcpy(hc + o_ppos, P.ppos.data(), (size_t)n_pad * 4);
    if ((rc = run.up(0, o_win))) return rc;
    const uint32_t mcap = (nP + 1) & ~1u;
    const size_t lds = (size_t)(mcap ? mcap : 2) * 12;

    EhhWin *h_wins = (EhhWin *)(hc + o_win);
    for (size_t c = 0; c < chunks.size(); ++c) {
        const uint64_t base = chunks[c].w_begin, cnt = chunks[c].w_end - base;
        uint32_t max_blk = 0, launches = 0;
        uint64_t words = 0;  // so far: every window's word offset inside its chunk
        for (uint64_t k = 0; k < cnt; ++k) {
            const impop_ehh_window &wv = windows[base + k];
            const uint32_t nb = nblk[base + k];
            h_wins[k] = EhhWin{wv.site_begin, wv.site_end, wv.core_site, words, (after_core ? wv.core_site + 1 : wv.site_begin) >> 6, nb, 0};
            max_blk = std::max(max_blk, nb);
            words += (uint64_t)nb * stride;
        }
        if ((rc = run.up(o_win, o_win + cnt * sizeof(EhhWin)))) return rc;
        if ((rc = run.timed(ctx->timers[impop_ctx::T_EHH], [&] {  // the chunk's kernels between two events of their own: impop_ctx_ehh_elapsed
            if (max_blk) {
                hipLaunchKernelGGL(ehh_scan_transpose_kernel, dim3((max_blk + 3) / 4, (uint32_t)cnt), dim3(256), 0, ctx->stream, m->d_sb,
                                   m->g.wps, m->g.G, m->g.r, (const EhhWin *)(dc + o_win), (const int32_t *)(dc + o_ppos), stride,
                                   (uint64_t *)(dc + o_wm));
                ++launches;
            }
            hipLaunchKernelGGL(ehh_refine_kernel, dim3((uint32_t)(cnt * 4)), dim3(EHH_ST), lds, ctx->stream, m->d_sb, m->g.wps, m->g.G,
                               m->g.r, (const EhhWin *)(dc + o_win), (const uint32_t *)(dc + o_idx), nP, mcap, params->flanks,
                               params->ref_hap, (const uint64_t *)(dc + o_wm), stride, (impop_ehh_stats *)(dc + o_rec), ctx->d_err);
            ++launches;
        }))) return rc;
        if (trace_on()) {
            fprintf(stderr, "[impop_ehh_scan] windows=%llu problems=%llu chunk=%llu launches=%u scratch_bytes=%llu\n",
                    (unsigned long long)cnt, (unsigned long long)(cnt * 4), (unsigned long long)c, launches, (unsigned long long)(words * 8));
            fflush(stderr);
        }
        if ((rc = run.finish(o_rec, o_rec + cnt * sizeof(impop_ehh_stats)))) return rc;
        const impop_ehh_stats *rv = (const impop_ehh_stats *)(hc + o_rec);
        for (uint64_t k = 0; k < cnt; ++k) {
            impop_ehh_stats o = rv[k];
            for (int a = 0; a < 2; ++a) o.area[a] = (double)(o.area_milli[a][0] + o.area_milli[a][1]) / 1000.0;
            out_host[base + k] = o;
        }
    }
    return IMPOP_OK;
}
