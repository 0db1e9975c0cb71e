// ihs.hip — impop_ihs_scan: per-site iHS / nSL / XP-EHH integrals from a positional Burrows-Wheeler transform on the device
// (include/impop_hip.h has the definitions, ihs_math.h the arithmetic shared with the host).
//
//   classify  one wave per 64-site block of d_sb (a compacted matrix: its kept sites, d_pos for their coordinates): c_P per
//             site -> the block's mask of stepped sites (0 < c_P < |P|, inside the site range) and of cores, and their counts
//   prefix    one workgroup: the counts -> the ordinal base and the core-index base of every block
//   tables    one wave per block: per stepped ordinal its coordinate, its column of d_sb and its core index (or none)
//   walk      grid = (chunks, 2 directions).  A workgroup carries the PBWT of P (order u16, divergence u32 in steps from its
//             warm-up start, both in LDS) over the stepped sites from the warm-up start of its chunk, and at every core of
//             its chunk turns the divergences of each class into the class's integrals: a break's nearest-greater spans give
//             the number of pairs whose match begins there, so the survivors at any step are a weighted count of breaks.
// A pair whose match began before the warm-up start carries divergence 0 and survives to every reach by construction
// (ihs_warm_start), so chunking never changes a byte.  Direction 0 writes half 0 of a record and its head, direction 1 half 1;
// flags are disjoint bits, ORed.  Every loop is bounded by a count from the tables; no flags or waits between workgroups.
#include <string.h>

#include <algorithm>
#include <vector>

#include "chunk_run.h"
#include "device_utils.h"
#include "ihs_math.h"
#include "internal.h"
#include "sb64.h"
#include "scan_route.h"
#include "win_chunks.h"

namespace impop {

constexpr int IHS_T = 256;
constexpr uint32_t IHS_NONE = 0xFFFFFFFFu;
__host__ __device__ inline uint32_t umin32(uint32_t a, uint32_t b) { return a < b ? a : b; }
__host__ __device__ inline uint64_t umin64(uint64_t a, uint64_t b) { return a < b ? a : b; }
static_assert(IMPOP_IHS_SCAN_MAX_N <= 16 * IHS_T && IMPOP_IHS_SCAN_MAX_N <= 65536, "a thread's strip fits 16 bits of a register; the order is u16");

struct IhsTables {
    const uint32_t *sb;
    const uint64_t *pos;            // compacted: the kept sites' original coordinates, else null
    const uint32_t *pm;             // wps dwords: the members of P
    uint64_t *step_mask, *core_mask;  // per block of the range
    uint32_t *step_cnt, *core_cnt;
    uint64_t *step_base, *core_base;  // n_blk + 1
    uint64_t *spos, *scol;          // per stepped ordinal; scol null: the column is the coordinate
    uint32_t *core_idx;
    uint64_t blk0, n_blk, cb, ce;   // the range's blocks and columns of d_sb
    uint64_t core_b, core_e;        // original coordinates
    uint32_t wps, G, r, nP, min_mac;
};

// grid = ceil(n_blk / 4): wave = one block, lane = one site
__global__ __launch_bounds__(256) void ihs_classify_kernel(const IhsTables A) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t bi = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (bi >= A.n_blk) return;  // wave-uniform
    const uint64_t B = A.blk0 + bi, col = B * 64 + lane;
    uint32_t c = 0;
    sb_for_each_dword<false>(A.sb + B * 64ull * A.wps, A.G, A.r, lane, [&](uint32_t k, uint32_t w) { c += __popc(w & A.pm[k]); });
    const bool in = col >= A.cb && col < A.ce;
    const uint64_t p = !in ? 0 : A.pos ? A.pos[col] : col;
    const bool stepped = in && c > 0 && c < A.nP;
    const uint32_t mac = c < A.nP - c ? c : A.nP - c;
    const bool core = stepped && p >= A.core_b && p < A.core_e && mac >= A.min_mac;
    const uint64_t sm = __ballot(stepped), cm = __ballot(core);
    if (lane == 0) {
        A.step_mask[bi] = sm;
        A.core_mask[bi] = cm;
        A.step_cnt[bi] = (uint32_t)__popcll(sm);
        A.core_cnt[bi] = (uint32_t)__popcll(cm);
    }
}

// one workgroup: exclusive prefix sums of both counts, the totals in entry n_blk
__global__ __launch_bounds__(1024) void ihs_prefix_kernel(const IhsTables A) {
    __shared__ uint64_t s_a[1024], s_b[1024];
    const uint32_t tid = threadIdx.x;
    const uint64_t per = (A.n_blk + 1023) / 1024;
    const uint64_t i0 = umin64(A.n_blk, tid * per), i1 = umin64(A.n_blk, i0 + per);
    uint64_t a = 0, b = 0;
    for (uint64_t i = i0; i < i1; ++i) {
        a += A.step_cnt[i];
        b += A.core_cnt[i];
    }
    s_a[tid] = a;
    s_b[tid] = b;
    __syncthreads();
    if (tid == 0) {
        uint64_t ra = 0, rb = 0;
        for (uint32_t t = 0; t < 1024; ++t) {
            const uint64_t ta = s_a[t], tb = s_b[t];
            s_a[t] = ra;
            s_b[t] = rb;
            ra += ta;
            rb += tb;
        }
        A.step_base[A.n_blk] = ra;
        A.core_base[A.n_blk] = rb;
    }
    __syncthreads();
    a = s_a[tid];
    b = s_b[tid];
    for (uint64_t i = i0; i < i1; ++i) {
        A.step_base[i] = a;
        A.core_base[i] = b;
        a += A.step_cnt[i];
        b += A.core_cnt[i];
    }
}

// grid = ceil(n_blk / 4): wave = one block; the stepped lanes write their ordinal's entries
__global__ __launch_bounds__(256) void ihs_tables_kernel(const IhsTables A) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t bi = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (bi >= A.n_blk) return;
    const uint64_t sm = A.step_mask[bi], cm = A.core_mask[bi], below = (1ull << lane) - 1ull;
    if (!((sm >> lane) & 1ull)) return;
    const uint64_t col = (A.blk0 + bi) * 64 + lane, o = A.step_base[bi] + (uint32_t)__popcll(sm & below);
    A.spos[o] = A.pos ? A.pos[col] : col;
    if (A.scol) A.scol[o] = col;
    A.core_idx[o] = ((cm >> lane) & 1ull) ? (uint32_t)(A.core_base[bi] + (uint32_t)__popcll(cm & below)) : IHS_NONE;
}

struct IhsWalk {
    const uint32_t *sb;
    const uint32_t *rows;           // member -> haplotype
    const uint8_t *lab;             // K = 2: member -> 0 (A) or 1 (B)
    const uint64_t *step_base, *core_base;
    const uint64_t *spos, *scol;    // scol == spos on a full matrix
    const uint32_t *core_idx;
    impop_ihs_core *rec;
    unsigned long long *steps;      // [0] all steps walked, [1] those before a chunk's own first stepped site
    uint32_t *err;
    IhsChunks ch;
    uint64_t n_st, max_bp, max_sites;
    uint32_t wps, G, r, n, nA, cutoff_milli;
};

// the workgroup's LDS, carved from the dynamic allocation
struct IhsLds {
    uint32_t *dv[2], *w, *hap, *gmax, *row[2];
    uint16_t *ord[2];
    uint8_t *lab;
};
inline size_t ihs_lds_bytes(uint32_t n, uint32_t wps) {
    return ((size_t)4 * n + ((n + 31) / 32 + 1) + 2 * (size_t)wps) * 4 + (size_t)2 * n * 2 + ((n + 3) & ~3u);
}

struct IhsScan {
    uint32_t z, f, v;
};
// workgroup-wide: totals of a and b in every thread.  s_red holds two sets of slots used in turn, so one barrier per call is
// enough: the set a call writes was last read two calls ago, in front of the barrier of the call in between.
__device__ inline void ihs_block_sum2(uint64_t &a, uint64_t &b, uint64_t (*s_red)[8], uint32_t &turn) {
    a = wave_sum_u64(a);
    b = wave_sum_u64(b);
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_red[turn][wave] = a;
        s_red[turn][4 + wave] = b;
    }
    __syncthreads();
    a = s_red[turn][0] + s_red[turn][1] + s_red[turn][2] + s_red[turn][3];
    b = s_red[turn][4] + s_red[turn][5] + s_red[turn][6] + s_red[turn][7];
    turn ^= 1u;
}

// the same for one 32-bit total (a probe of the search: at most C_g < 2^23)
__device__ inline uint32_t ihs_block_sum(uint32_t a, uint32_t (*s_red32)[4], uint32_t &turn) {
    a = wave_sum_u32(a);
    if ((threadIdx.x & 63) == 0) s_red32[turn][threadIdx.x >> 6] = a;
    __syncthreads();
    a = s_red32[turn][0] + s_red32[turn][1] + s_red32[turn][2] + s_red32[turn][3];
    turn ^= 1u;
    return a;
}

// Stable partition of the order by bit(member) with the divergences carried: an element's new predecessor is the last earlier
// element with its bit, and everything between the two has the other bit, so its new divergence is the maximum over the run
// in front of it and itself.  Runs are joined across the threads' strips by a segmented maximum scan.  The first element of
// either side gets `sentinel`.  Returns the number of zeros.  The caller puts a barrier behind it.
template <typename BitF>
__device__ inline uint32_t ihs_partition(const uint16_t *so, const uint32_t *sd, uint16_t *dO, uint32_t *dd, uint32_t n, uint32_t sentinel,
                                         BitF bit, IhsScan *s_scan) {
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t E = (n + IHS_T - 1) / IHS_T, i0 = umin32(n, tid * E), i1 = umin32(n, i0 + E);
    const uint32_t prevb = (i0 > 0 && i0 < n) ? bit(so[i0 - 1]) : 2u;
    uint32_t bits = 0, z = 0, f = 0, v = 0, pb = prevb;
    for (uint32_t i = i0; i < i1; ++i) {
        const uint32_t b = bit(so[i]), d = sd[i];
        bits |= b << (i - i0);
        z += b ^ 1u;
        if (b != pb) {
            f = 1;
            v = d;
        } else v = v > d ? v : d;
        pb = b;
    }
    // inclusive scan inside the wave: (z: sum), (f, v): segmented maximum, the later operand on the right
    uint32_t zi = z, fi = f, vi = v;
#pragma unroll
    for (uint32_t off = 1; off < 64; off <<= 1) {
        const uint32_t z2 = __shfl_up(zi, off, 64), f2 = __shfl_up(fi, off, 64), v2 = __shfl_up(vi, off, 64);
        if (lane >= off) {
            zi += z2;
            if (!fi) vi = vi > v2 ? vi : v2;
            fi |= f2;
        }
    }
    if (lane == 63) s_scan[wave] = {zi, fi, vi};
    // exclusive inside the wave
    uint32_t ze = __shfl_up(zi, 1, 64), fe = __shfl_up(fi, 1, 64), ve = __shfl_up(vi, 1, 64);
    if (lane == 0) ze = fe = ve = 0;
    __syncthreads();
    uint32_t zb = 0, vb = 0, Z = 0;  // the waves in front of this one
    for (uint32_t k = 0; k < IHS_T / 64; ++k) {
        const IhsScan t = s_scan[k];
        Z += t.z;
        if (k < wave) {
            zb += t.z;
            vb = t.f ? t.v : (vb > t.v ? vb : t.v);
        }
    }
    const uint32_t zpre = zb + ze;
    uint32_t rm = fe ? ve : (vb > ve ? vb : ve);  // the maximum of the run that ends in front of the strip
    uint32_t zc = zpre;
    pb = prevb;
    for (uint32_t i = i0; i < i1; ++i) {
        const uint32_t b = (bits >> (i - i0)) & 1u, d = sd[i];
        uint32_t nd = d;
        if (b != pb) {
            nd = d > rm ? d : rm;
            rm = d;
        } else rm = rm > d ? rm : d;
        pb = b;
        const uint32_t np = b ? Z + (i - zc) : zc;
        zc += b ^ 1u;
        if (np == 0 || np == Z) nd = sentinel;
        dO[np] = so[i];
        dd[np] = nd;
    }
    return Z;
}

// grid = (chunks, 2), dynamic LDS = ihs_lds_bytes(n, wps)
template <bool K2>
__global__ __launch_bounds__(IHS_T) void ihs_walk_kernel(const IhsWalk A) {
    extern __shared__ uint32_t ihs_lds[];
    __shared__ IhsScan s_scan[IHS_T / 64];
    __shared__ uint64_t s_red[2][8];
    __shared__ uint32_t s_red32[2][4];
    const uint32_t tid = threadIdx.x, n = A.n, wps = A.wps;
    const int dir = (int)blockIdx.y;
    const uint64_t b0 = A.ch.begin(blockIdx.x), b1 = A.ch.end(blockIdx.x);
    if (A.core_base[b1] == A.core_base[b0]) return;  // no core of its own: nothing to write (workgroup-uniform)
    const uint64_t o0 = A.step_base[b0], o1 = A.step_base[b1], n_st = A.n_st;
    auto pos = [&](uint64_t i) { return A.spos[i]; };
    const uint64_t ws = ihs_warm_start(dir, o0, o1, n_st, A.max_bp, A.max_sites, pos);
    const uint64_t n_steps64 = dir ? ws - o0 + 1 : o1 - ws;
    const uint32_t n_steps = (uint32_t)n_steps64;  // the host refuses ranges of 2^32 sites
    auto ordinal = [&](uint32_t step) { return dir ? ws - step : ws + step; };
    if (tid == 0) {
        atomicAdd(A.steps, (unsigned long long)n_steps);
        atomicAdd(A.steps + 1, (unsigned long long)(dir ? ws - (o1 - 1) : o0 - ws));
    }

    IhsLds L;
    {
        uint32_t *p = ihs_lds;
        L.dv[0] = p; p += n;
        L.dv[1] = p; p += n;
        L.w = p; p += n;
        L.hap = p; p += n;
        L.gmax = p; p += (n + 31) / 32 + 1;
        L.row[0] = p; p += wps;
        L.row[1] = p; p += wps;
        L.ord[0] = reinterpret_cast<uint16_t *>(p);
        L.ord[1] = L.ord[0] + n;
        L.lab = reinterpret_cast<uint8_t *>(L.ord[1] + n);
    }
    for (uint32_t i = tid; i < n; i += IHS_T) {
        L.ord[0][i] = (uint16_t)i;
        L.dv[0][i] = 0;
        L.hap[i] = A.rows[i];
        if (K2) L.lab[i] = A.lab[i];
    }
    auto load_row = [&](uint64_t col, uint32_t k) { return A.sb[sb_index(wps, A.G, A.r, col >> 6, (uint32_t)(col & 63), k)]; };
    {
        const uint64_t col = A.scol[ws];
        for (uint32_t k = tid; k < wps; k += IHS_T) L.row[0][k] = load_row(col, k);
    }
    // one step ahead: the next site's column and core index
    uint64_t col_next = n_steps > 1 ? A.scol[ordinal(1)] : 0;
    uint32_t ci = A.core_idx[ws];
    uint32_t turn = 0, turn32 = 0, cur = 0;
    uint64_t far_bp = 0;  // the base-pair reach of the last core, carried along the walk
    bool have_far = false;
    __syncthreads();

    for (uint32_t s = 0; s < n_steps; ++s) {
        const uint64_t x = ordinal(s);
        const uint32_t *row = L.row[s & 1];
        const bool more = s + 1 < n_steps;
        uint32_t pre = 0, ci_next = IHS_NONE;
        if (more) {
            if (tid < wps) pre = load_row(col_next, tid);
            ci_next = A.core_idx[ordinal(s + 1)];
        }
        const uint64_t col_next2 = s + 2 < n_steps ? A.scol[ordinal(s + 2)] : 0;
        auto site_bit = [&](uint32_t member) {
            const uint32_t h = L.hap[member];
            return (row[h >> 5] >> (h & 31)) & 1u;
        };
        const uint32_t Z = ihs_partition(L.ord[cur], L.dv[cur], L.ord[cur ^ 1], L.dv[cur ^ 1], n, s + 1, site_bit, s_scan);
        if (more) {
            uint32_t *nrow = L.row[(s + 1) & 1];
            if (tid < wps) nrow[tid] = pre;
            for (uint32_t k = tid + IHS_T; k < wps; k += IHS_T) nrow[k] = load_row(col_next, k);
        }
        cur ^= 1;
        __syncthreads();

        const bool own = dir ? x < o1 : x >= o0;
        if (ci != IHS_NONE && own) {  // workgroup-uniform
            // the classes as ranges of one order: by allele they are the PBWT's own two sides; by population the order is
            // partitioned once more, by label, into the buffers the step has just left
            const uint16_t *CO = L.ord[cur];
            const uint32_t *CD = L.dv[cur];
            uint32_t split = Z;
            uint64_t c1a = 0, c1b = 0;
            if (K2) {
                auto label = [&](uint32_t member) { return (uint32_t)L.lab[member]; };
                split = ihs_partition(L.ord[cur], L.dv[cur], L.ord[cur ^ 1], L.dv[cur ^ 1], n, s + 1, label, s_scan);
                __syncthreads();
                CO = L.ord[cur ^ 1];
                CD = L.dv[cur ^ 1];
                for (uint32_t i = tid; i < n; i += IHS_T)
                    if (site_bit(CO[i])) (i < split ? c1a : c1b) += 1;
                ihs_block_sum2(c1a, c1b, s_red, turn);
            } else {
                c1b = n - Z;
            }
            for (uint32_t g = tid; g < (n + 31) / 32; g += IHS_T) {
                uint32_t mx = 0;
                for (uint32_t i = g * 32; i < umin32(n, g * 32 + 32); ++i) mx = mx > CD[i] ? mx : CD[i];
                L.gmax[g] = mx;
            }
            __syncthreads();
            auto dval = [&](uint32_t i) { return CD[i]; };
            auto gm = [&](uint32_t g) { return L.gmax[g]; };
            // the reach of either measure from this core, in steps
            far_bp = have_far ? ihs_far_advance(dir, far_bp, x, n_st, A.max_bp, pos) : ihs_far(dir, 0, x, n_st, A.max_bp, pos);
            have_far = true;
            const uint64_t far[2] = {far_bp, ihs_far(dir, 1, x, n_st, A.max_sites, pos)};
            uint32_t lb[2];
            bool bad = false;
            for (int m = 0; m < 2; ++m) {
                const uint64_t J = dir ? far[m] - x : x - far[m];
                bad = bad || J > s;
                lb[m] = J > s ? 0u : s - (uint32_t)J;
            }
            const uint32_t lbmin = lb[0] < lb[1] ? lb[0] : lb[1];
            const uint64_t pk = A.spos[x];
            impop_ihs_core *rec = A.rec + ci;
            if (tid == 0 && dir == 0) {
                rec->site = pk;
                rec->n[0] = split;
                rec->n[1] = n - split;
                rec->c1[0] = (uint32_t)c1a;
                rec->c1[1] = (uint32_t)c1b;
            }
            uint32_t flags = 0;
            for (int g = 0; g < 2; ++g) {
                const uint32_t lo = g ? split : 0, hi = g ? n : split, ng = hi - lo;
                if (ng < 2) continue;
                const uint64_t C = (uint64_t)ng * (ng - 1) / 2;
                for (uint32_t t = lo + 1 + tid; t < hi; t += IHS_T)
                    L.w[t] = ihs_span_left(t, lo + 1, hi, dval, gm) * ihs_span_right(t, lo + 1, hi, dval, gm);
                __syncthreads();
                // pairs whose match begins behind step xx
                auto broken_after = [&](uint32_t xx) {
                    uint32_t a = 0;
                    for (uint32_t t = lo + 1 + tid; t < hi; t += IHS_T)
                        if (CD[t] > xx) a += L.w[t];
                    return (uint64_t)ihs_block_sum(a, s_red32, turn32);
                };
                uint32_t all = 0;
                for (uint32_t t = lo + 1 + tid; t < hi; t += IHS_T) all += L.w[t];
                bad = bad || ihs_block_sum(all, s_red32, turn32) != C;
                if (ihs_cut_ok(C - broken_after(s), C, A.cutoff_milli)) {
                    // the smallest step at which the cutoff still holds; the farthest reach first: it answers at once where the
                    // curve never falls to the cutoff
                    uint32_t xl = lbmin, xh = s;
                    if (xl < xh && !ihs_cut_ok(C - broken_after(xl), C, A.cutoff_milli)) {
                        ++xl;
                        while (xl < xh) {
                            const uint32_t mid = xl + (xh - xl) / 2;
                            if (ihs_cut_ok(C - broken_after(mid), C, A.cutoff_milli)) xh = mid;
                            else xl = mid + 1;
                        }
                    }
                    for (int m = 0; m < 2; ++m) {
                        const uint32_t e = xl > lb[m] ? xl : lb[m];
                        auto U = [&](uint32_t step) -> uint64_t {
                            if (m) return s - step;
                            const uint64_t p = A.spos[ordinal(step)];
                            return p > pk ? p - pk : pk - p;
                        };
                        uint64_t a = 0, b = 0;
                        for (uint32_t t = lo + 1 + tid; t < hi; t += IHS_T) {
                            const uint32_t d = CD[t];
                            if (d > e) {
                                a += L.w[t];
                                if (d <= s) b += ihs_break_term(L.w[t], d, s, U(d), U(d - 1));
                            }
                        }
                        ihs_block_sum2(a, b, s_red, turn);
                        const uint64_t I2 = ihs_alive_term(C - a, U(e)) + b;
                        if (tid == 0) (m ? rec->sl2 : rec->ihh2)[g][dir] = I2;
                        flags |= ihs_flag(m, g, dir, e == lb[m], ihs_far_is_edge(dir, far[m], n_st));
                    }
                }
                __syncthreads();  // L.w is rewritten for the next class
            }
            if (tid == 0) {
                if (flags) atomicOr(&rec->flags, flags);
                if (bad) atomicOr(A.err, DEV_ERR_IHS);
            }
        }
        ci = ci_next;
        col_next = col_next2;
    }
}

}  // namespace impop

using namespace impop;

IMPOP_API int impop_ihs_scan(impop_ctx *ctx, const impop_matrix *m, uint64_t site_begin, uint64_t site_end, uint64_t core_begin,
                             uint64_t core_end, const uint64_t *mask_a, const uint64_t *mask_b, const impop_ihs_params *params,
                             impop_ihs_core *out_host, uint64_t capacity, uint64_t *n_cores) {
    static_assert(sizeof(impop_ihs_params) == 32 && sizeof(impop_ihs_core) == 96, "ABI layout");
    const char *fn = "impop_ihs_scan";
    REQUIRE(ctx && m && params && n_cores, "%s: NULL argument", fn);
    REQUIRE(params->struct_size == sizeof(impop_ihs_params), "impop_ihs_params.struct_size mismatch");
    REQUIRE(m->device == ctx->device, "%s: matrix lives on device %d, context on %d", fn, m->device, ctx->device);
    REQUIRE(params->min_mac >= 1, "%s: min_mac must be at least 1", fn);
    REQUIRE(params->cutoff_milli <= 1000, "%s: cutoff_milli %u is above 1000", fn, params->cutoff_milli);
    const uint64_t span = matrix_span(m), b = site_begin, e = site_end ? site_end : span;
    REQUIRE(b < e && e <= span, "%s: bad site range [%llu,%llu) for %llu sites", fn, (unsigned long long)b, (unsigned long long)e,
            (unsigned long long)span);
    REQUIRE(e - b < (1ull << 32), "%s: a range of %llu sites does not fit the 32-bit step counts", fn, (unsigned long long)(e - b));
    const uint64_t kb = core_begin, ke = core_end ? core_end : e;
    REQUIRE(b <= kb && kb <= ke && ke <= e, "%s: core range [%llu,%llu) is not inside the site range [%llu,%llu)", fn, (unsigned long long)kb,
            (unsigned long long)ke, (unsigned long long)b, (unsigned long long)e);
    REQUIRE(!(mask_b && !mask_a), "%s: mask_b without mask_a", fn);
    const uint32_t nh = m->g.n_hap, wps = m->g.wps, K = mask_b ? 2 : 1;
    const uint32_t mwords = (nh + 63) / 64;
    std::vector<uint64_t> uni;
    MemberSet RA;
    if (K == 2) {
        uni.resize(mwords);
        for (uint32_t i = 0; i < mwords; ++i) {
            const uint64_t valid = (i + 1 == mwords && (nh & 63)) ? (1ull << (nh & 63)) - 1ull : ~0ull;
            REQUIRE((mask_a[i] & mask_b[i] & valid) == 0, "%s: the two populations share a haplotype", fn);
            uni[i] = (mask_a[i] | mask_b[i]) & valid;
        }
        RA = member_set(mask_a, nh, wps);
        const MemberSet RB = member_set(mask_b, nh, wps);
        REQUIRE(RA.size() >= 2 && RB.size() >= 2, "%s: populations of %u and %u members; each needs at least 2", fn, RA.size(), RB.size());
    }
    const MemberSet R = member_set(K == 2 ? uni.data() : mask_a, nh, wps);
    const uint32_t n = R.size();
    REQUIRE(n >= 2, "%s: %u members make no pair", fn, n);
    if (n > IMPOP_IHS_SCAN_MAX_N) {
        set_error("%s: %u members exceed the limit (%u)", fn, n, (uint32_t)IMPOP_IHS_SCAN_MAX_N);
        return IMPOP_E_UNSUPPORTED;
    }
    const size_t lds = ihs_lds_bytes(n, wps);
    if (lds > 150 * 1024) {
        set_error("%s: %u haplotypes per site need more LDS than a workgroup has", fn, nh);
        return IMPOP_E_UNSUPPORTED;
    }

    // the range's columns of d_sb and their blocks
    const uint64_t cb = m->compact ? pos_lower_bound(m, b) : b, ce = m->compact ? pos_lower_bound(m, e) : e;
    const uint64_t blk0 = cb >> 6, n_blk = ce > cb ? ((ce + 63) >> 6) - blk0 : 0;
    uint64_t n_st = 0, total = 0, launches = 0, n_chunks = 0;
    unsigned long long steps[2] = {0, 0};
    auto trace = [&]() {
        if (!trace_on()) return;
        fprintf(stderr, "[impop_ihs_scan] route=%s pops=%u members=%u stepped=%llu cores=%llu chunks=%llu warmup_steps=%llu launches=%llu bytes_streamed=%llu\n",
                m->compact ? "compact" : "dense", K, n, (unsigned long long)n_st, (unsigned long long)total, (unsigned long long)n_chunks,
                steps[1], (unsigned long long)launches, (unsigned long long)((n_blk * 64 + steps[0]) * wps * 4));
        fflush(stderr);
    };
    *n_cores = 0;
    if (n_blk == 0) {
        trace();
        return IMPOP_OK;
    }

    // device, first part: masks | rows | labels | per-block masks, counts and bases
    std::vector<uint8_t> lab(n, 0);
    if (K == 2)
        for (uint32_t i = 0; i < n; ++i) lab[i] = RA.ppos[R.idx[i]] >= 0 ? 0 : 1;
    Carve L;
    const size_t o_pm = L.take<uint32_t>(wps), o_rows = L.take<uint32_t>(n), o_lab = L.take<uint8_t>(n),
                 o_smask = L.take<uint64_t>(n_blk), o_cmask = L.take<uint64_t>(n_blk), o_scnt = L.take<uint32_t>(n_blk),
                 o_ccnt = L.take<uint32_t>(n_blk), o_sbase = L.take<uint64_t>(n_blk + 1), o_cbase = L.take<uint64_t>(n_blk + 1),
                 o_steps = L.take<unsigned long long>(2);
    HIP_TRY(hipSetDevice(ctx->device));
    void *d = nullptr;
    int rc = ctx_scratch(ctx, L.total(), &d);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemcpyAsync(L.at<char>(d, o_pm), R.bits.data(), (size_t)wps * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(L.at<char>(d, o_rows), R.idx.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(L.at<char>(d, o_lab), lab.data(), (size_t)n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(L.at<char>(d, o_steps), 0, 16, st));

    IhsTables T{};
    T.sb = m->d_sb;
    T.pos = m->compact ? m->d_pos : nullptr;
    T.pm = L.at<uint32_t>(d, o_pm);
    T.step_mask = L.at<uint64_t>(d, o_smask);
    T.core_mask = L.at<uint64_t>(d, o_cmask);
    T.step_cnt = L.at<uint32_t>(d, o_scnt);
    T.core_cnt = L.at<uint32_t>(d, o_ccnt);
    T.step_base = L.at<uint64_t>(d, o_sbase);
    T.core_base = L.at<uint64_t>(d, o_cbase);
    T.blk0 = blk0;
    T.n_blk = n_blk;
    T.cb = cb;
    T.ce = ce;
    T.core_b = kb;
    T.core_e = ke;
    T.wps = wps;
    T.G = m->g.G;
    T.r = m->g.r;
    T.nP = n;
    T.min_mac = params->min_mac;

    EventPairs *timer = ctx->timers + impop_ctx::T_IHS;
    const dim3 blk_grid((uint32_t)((n_blk + 3) / 4));
    if ((rc = timed(ctx, timer[0], [&] {
            hipLaunchKernelGGL(ihs_classify_kernel, blk_grid, dim3(256), 0, st, T);
            hipLaunchKernelGGL(ihs_prefix_kernel, dim3(1), dim3(1024), 0, st, T);
        })))
        return rc;
    launches += 2;
    uint64_t totals[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&totals[0], T.step_base + n_blk, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&totals[1], T.core_base + n_blk, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    n_st = totals[0];
    total = totals[1];
    *n_cores = total;
    if (total == 0 || !out_host || capacity < total) {  // the count alone
        trace();
        return IMPOP_OK;
    }

    // second part, in a side buffer so that the first stays where it is: the stepped sites' tables and the records
    Carve L2;
    const size_t o_spos = L2.take<uint64_t>(n_st), o_scol = L2.take<uint64_t>(m->compact ? n_st : 0), o_cidx = L2.take<uint32_t>(n_st),
                 o_rec = L2.take<impop_ihs_core>(total);
    void *d2 = nullptr;
    if ((rc = ctx_aux(ctx, 0, L2.total() + 256, &d2))) return rc;
    T.spos = L2.at<uint64_t>(d2, o_spos);
    T.scol = m->compact ? L2.at<uint64_t>(d2, o_scol) : nullptr;
    T.core_idx = L2.at<uint32_t>(d2, o_cidx);
    HIP_TRY(hipMemsetAsync(L2.at<char>(d2, o_rec), 0, total * sizeof(impop_ihs_core), st));
    if ((rc = timed(ctx, timer[0], [&] { hipLaunchKernelGGL(ihs_tables_kernel, blk_grid, dim3(256), 0, st, T); }))) return rc;
    ++launches;

    IhsWalk W{};
    W.sb = m->d_sb;
    W.rows = L.at<uint32_t>(d, o_rows);
    W.lab = L.at<uint8_t>(d, o_lab);
    W.step_base = T.step_base;
    W.core_base = T.core_base;
    W.spos = T.spos;
    W.scol = m->compact ? T.scol : T.spos;
    W.core_idx = T.core_idx;
    W.rec = L2.at<impop_ihs_core>(d2, o_rec);
    W.steps = L.at<unsigned long long>(d, o_steps);
    W.err = ctx->d_err;
    W.ch = ihs_chunks(n_blk, n_st, e - b, params->max_extend_bp, params->max_extend_sites, env_tile_blocks("IMPOP_IHS_CHUNK_BLOCKS"),
                      (uint32_t)ctx->n_cu);
    W.n_st = n_st;
    W.max_bp = params->max_extend_bp;
    W.max_sites = params->max_extend_sites;
    W.wps = wps;
    W.G = m->g.G;
    W.r = m->g.r;
    W.n = n;
    W.nA = K == 2 ? RA.size() : 0;
    W.cutoff_milli = params->cutoff_milli;
    n_chunks = W.ch.count();
    REQUIRE(n_chunks < (1ull << 31), "%s: %llu chunks exceed a launch", fn, (unsigned long long)n_chunks);
    if ((rc = lds_opt_in(K == 2 ? ihs_walk_kernel<true> : ihs_walk_kernel<false>, lds))) return rc;
    if ((rc = timed(ctx, timer[1], [&] {
            const dim3 grid((uint32_t)n_chunks, 2);
            if (K == 2) hipLaunchKernelGGL(ihs_walk_kernel<true>, grid, dim3(IHS_T), lds, st, W);
            else hipLaunchKernelGGL(ihs_walk_kernel<false>, grid, dim3(IHS_T), lds, st, W);
        })))
        return rc;
    ++launches;
    HIP_TRY(hipMemcpyAsync(out_host, W.rec, total * sizeof(impop_ihs_core), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(steps, W.steps, 16, hipMemcpyDeviceToHost, st));
    if ((rc = ctx_err_fetch(ctx))) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    if ((rc = ctx_err_result(ctx, fn))) return rc;
    trace();
    return IMPOP_OK;
}

IMPOP_API int impop_ctx_ihs_elapsed(impop_ctx *ctx, double kernel_ms[2], uint64_t *calls) {
    REQUIRE(ctx && kernel_ms, "impop_ctx_ihs_elapsed: NULL argument");
    return ctx_timers_elapsed(ctx, impop_ctx::T_IHS, 2, 1, kernel_ms, calls);
}
