// ===========================================================================
// affine_sums.hpp -- what the data terms on the matrix of an AFFINE lattice share (ssd_affine.hip, mi_affine.hip): the value and
// the gradient of one stencil, the NS sums of a Gauss-Newton step held in double, their two organisations, the fixed-order
// reduction and the finish, and the validation of the problem.  A data term supplies its per-sample terms as a functor
//
//     terms(o, od, lt, q, h):   od = (o_0 .. o_{D-1}, 1) as doubles,  lt the loss term,  q[d],  h[pair(d, d')] (HESS), formed in R
//
// and the sums are
//     [0]                                    lt
//     [1 + d (D+1) + e]                      q_d o~_e
//     [1 + P + pair(d,d') M + pair(e,e')]    h_dd' o~_e o~_e',   M = (D+1)(D+2)/2 moments, pair: upper triangle row by row
// NS = 1 + P + D(D+1)/2 * M: 73 / 25 / 6 for D = 3 / 2 / 1; without a Hessian 1 + P.  (o~_e o~_e' is exact in double whenever it is
// below 2^53.)  No atomics, nothing in the workspace is assumed cleared: the summation tree depends on the shape alone.
// ===========================================================================
#pragma once
#include "../../include/interpol_hip.h"
#include "regulariser_at.hpp"                                      // ops_generic.hpp, ranges_overlap
#include <hip/hip_runtime.h>
#include <string.h>

namespace ip {
namespace ssd_affine {

// Persistent workgroups of the partial sums per batch item = doubles per sum and item in the workspace.  A CONSTANT.
constexpr int SA_BLOCKS = 1024;
constexpr int WAVES = BLOCK / 64;
constexpr int FINISH_WAYS = SA_BLOCKS / 64;                         // the doubles of one sum that one lane of the finish adds

constexpr int params(int D) { return D * (D + 1); }
constexpr int moments(int D) { return (D + 1) * (D + 2) / 2; }
constexpr int num_sums(int D, bool hess) { return 1 + params(D) + (hess ? (D * (D + 1) / 2) * moments(D) : 0); }
// index of (i, j), i <= j < n, in the upper triangle of an n x n matrix, row by row
__host__ __device__ constexpr int pair_index(int i, int j, int n) { return i * n - i * (i - 1) / 2 + (j - i); }

// One channel under the stencil `s`: aw = sum_taps W v, av[d] = sum_taps dW/dx_d v (before the mask).
template <typename R, int D, int KMAX>
__device__ __forceinline__ void stencil_value_gradient(const KParams &p, Stencil<R, D, KMAX, true, NEED_G> &s, const R *v0, R &aw, R *av)
{
    opaque(s);
    R a0 = R(0), a1 = R(0), a2 = R(0);
    aw = R(0);
    IP_FOR_I {
        R pWW = R(0), pGW = R(0), pWG = R(0);
        IP_FOR_J {
            const unsigned oij = s.off[0][i] + s.off[1][j];
            R rW = R(0), rG = R(0);
            IP_FOR_K {
                const R v = ld_tap(v0, oij + s.off[2][k]);
                rW = fma_(s.w[2][k], v, rW);
                if (D > 2) rG = fma_(s.g[2][k], v, rG);
            } IP_ROW_END;
            pWW = fma_(s.w[1][j], rW, pWW);
            if (D > 1) pGW = fma_(s.g[1][j], rW, pGW);
            if (D > 2) pWG = fma_(s.w[1][j], rG, pWG);
        }
        aw = fma_(s.w[0][i], pWW, aw);
        a0 = fma_(s.g[0][i], pWW, a0);
        if (D > 1) a1 = fma_(s.w[0][i], pGW, a1);
        if (D > 2) a2 = fma_(s.w[0][i], pWG, a2);
    }
    av[0] = a0; av[1] = a1; av[2] = a2;
}

// od = (o_0 .. o_{D-1}, 1) as doubles (the split of load_coords)
template <int D>
__device__ __forceinline__ void sample_index(const KParams &p, int64_t o, double *od)
{
    unsigned rr = (unsigned)o;
#pragma unroll
    for (int d = D - 1; d > 0; --d) { const unsigned qq = rr / (unsigned)p.gshape[d]; od[d] = (double)(rr - qq * (unsigned)p.gshape[d]); rr = qq; }
    od[0] = (double)rr;
    od[D] = 1.0;
}

// SA_BLOCKS persistent workgroups per batch item, the item `b` on gridDim.y.  A workgroup takes runs of BLOCK consecutive samples,
// SA_BLOCKS runs apart; every term is converted to double ONCE and multiplied into the NS sums held in double in registers.  One
// fixed-order workgroup reduction at the end (lanes by halving shuffles, then the waves in turn); every workgroup writes its NS
// doubles, also when it met no sample: sums[b][i][workgroup].
template <typename R, int D, bool HESS, typename Terms>
__device__ __forceinline__ void partial_sums(const KParams &p, const Terms &terms, double *__restrict__ sums, int64_t b)
{
    constexpr int P = params(D), M = moments(D), NS = num_sums(D, HESS), K = D * (D + 1) / 2;
    __shared__ double part[WAVES][NS];
    double acc[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) acc[i] = 0.0;
    for (int64_t o = (int64_t)blockIdx.x * BLOCK + threadIdx.x; o < p.N; o += (int64_t)SA_BLOCKS * BLOCK) {
        double od[D + 1];
        R lt, q[D], h[K];
        terms(o, od, lt, q, h);
        // one conversion to double each
        acc[0] += (double)lt;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const double qd = (double)q[d];
#pragma unroll
            for (int e = 0; e <= D; ++e) acc[1 + d * (D + 1) + e] = __builtin_fma(qd, od[e], acc[1 + d * (D + 1) + e]);
        }
        if (HESS) {
            double mo[M];
#pragma unroll
            for (int e = 0; e <= D; ++e) {
#pragma unroll
                for (int f = e; f <= D; ++f) mo[pair_index(e, f, D + 1)] = f == D ? od[e] : od[e] * od[f];
            }
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const double hk = (double)h[k];
#pragma unroll
                for (int m = 0; m < M; ++m) acc[1 + P + k * M + m] = __builtin_fma(hk, mo[m], acc[1 + P + k * M + m]);
            }
        }
    }
    // the workgroup's sums in a fixed order: lanes by halving shuffles, then the waves one after the other
#pragma unroll
    for (int i = 0; i < NS; ++i) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc[i] += __shfl_down(acc[i], off, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NS; ++i) part[wave][i] = acc[i];
    }
    __syncthreads();
    if (threadIdx.x < NS) {
        double t = part[0][threadIdx.x];
        for (int w = 1; w < WAVES; ++w) t += part[w][threadIdx.x];
        sums[(b * NS + threadIdx.x) * SA_BLOCKS + blockIdx.x] = t;
    }
}

// The other organisation of the same sums, for the instantiations whose NS accumulators leave one wave per SIMD (3-D with a
// Hessian: 256 VGPRs + 42..58 AGPRs): the 1 + D + K terms and the D + 1 indices of a run of BLOCK samples go through LDS as doubles
// (a record of REC doubles per sample), and thread (i, j) = (sum, j-th part of the run) adds its sum over its samples -- one
// accumulator per thread instead of NS, 82..176 VGPRs, 2..5 waves per SIMD, 30 KiB of LDS.  GROUPS = BLOCK / NS parts (3 in 3-D:
// 219 of the 256 threads add).  The parts are added in turn at the end.
template <typename R, int D, typename Terms>
__device__ __forceinline__ void partial_sums_staged(const KParams &p, const Terms &terms, double *__restrict__ sums, int64_t b)
{
    constexpr int P = params(D), M = moments(D), NS = num_sums(D, true), K = D * (D + 1) / 2;
    constexpr int NV = 1 + D + K, REC = NV + D + 1, GROUPS = BLOCK / NS, PER = (BLOCK + GROUPS - 1) / GROUPS;
    static_assert(GROUPS >= 1, "one thread per sum at least");
    __shared__ double stage[BLOCK * REC];
    __shared__ double part[GROUPS][NS];
    // which term and which two indices this thread multiplies
    const int grp = threadIdx.x / NS, own = threadIdx.x - grp * NS;
    int vi = 0, ea = D, eb = D;
    if (own >= 1 && own < 1 + P) { vi = 1 + (own - 1) / (D + 1); ea = (own - 1) % (D + 1); }
    if (own >= 1 + P) {
        const int k = (own - 1 - P) / M, m = (own - 1 - P) - k * M;
        vi = 1 + D + k;
        for (int e = 0; e <= D; ++e)
            for (int f = e; f <= D; ++f)
                if (pair_index(e, f, D + 1) == m) { ea = e; eb = f; }
    }
    const int s0 = grp * PER, s1 = grp < GROUPS ? (s0 + PER < BLOCK ? s0 + PER : BLOCK) : s0;
    double acc = 0.0;
    for (int64_t base = (int64_t)blockIdx.x * BLOCK; base < p.N; base += (int64_t)SA_BLOCKS * BLOCK) {
        const int64_t o = base + threadIdx.x;
        double *rec = stage + threadIdx.x * REC;
        if (o < p.N) {
            double od[D + 1];
            R lt, q[D], h[K];
            terms(o, od, lt, q, h);
            rec[0] = (double)lt;
#pragma unroll
            for (int d = 0; d < D; ++d) rec[1 + d] = (double)q[d];
#pragma unroll
            for (int k = 0; k < K; ++k) rec[1 + D + k] = (double)h[k];
#pragma unroll
            for (int e = 0; e <= D; ++e) rec[NV + e] = od[e];
        } else {
#pragma unroll
            for (int v = 0; v < REC; ++v) rec[v] = 0.0;
        }
        __syncthreads();
#pragma unroll 4
        for (int s = s0; s < s1; ++s) {
            const double *r = stage + s * REC;
            acc = __builtin_fma(r[vi], r[NV + ea] * r[NV + eb], acc);
        }
        __syncthreads();
    }
    if (grp < GROUPS) part[grp][own] = acc;
    __syncthreads();
    if (threadIdx.x < NS) {
        double t = part[0][threadIdx.x];
        for (int g = 1; g < GROUPS; ++g) t += part[g][threadIdx.x];
        sums[(b * NS + threadIdx.x) * SA_BLOCKS + blockIdx.x] = t;
    }
}

// The finish of item `b` by one workgroup: wave w sums the SA_BLOCKS doubles of the sums i = w, w + 4, ..: 16 independent partial
// sums per lane, folded in a fixed order, then the lanes by halving shuffles.  tot[NS] (shared) holds the sums after the barrier.
template <int D, bool HESS>
__device__ __forceinline__ void finish_sums(const double *__restrict__ sums, int64_t b, double *tot)
{
    constexpr int NS = num_sums(D, HESS);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = wave; i < NS; i += WAVES) {
        // FINISH_WAYS independent loads per lane, folded pairwise: which double goes into which sum is fixed
        const double *col = sums + (b * NS + i) * SA_BLOCKS;
        double a[FINISH_WAYS];
#pragma unroll
        for (int j = 0; j < FINISH_WAYS; ++j) a[j] = col[lane + 64 * j];
#pragma unroll
        for (int w = FINISH_WAYS / 2; w > 0; w /= 2) {
#pragma unroll
            for (int j = 0; j < w; ++j) a[j] += a[j + w];
        }
        double t = a[0];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
        if (lane == 0) tot[i] = t;
    }
    __syncthreads();
}

// tot -> gradient (B, D, D+1), hessian (B, P, P): BOTH triangles of the Hessian from the same sum (exactly symmetric), in R
template <typename R, int D, bool HESS>
__device__ __forceinline__ void write_gradient_hessian(const double *tot, int64_t b, R *__restrict__ gradient, R *__restrict__ hessian)
{
    constexpr int P = params(D), M = moments(D);
    if (threadIdx.x < P) gradient[b * P + threadIdx.x] = (R)tot[1 + threadIdx.x];
    if (HESS) {
        for (int t = threadIdx.x; t < P * P; t += BLOCK) {
            const int row = t / P, col = t - row * P;
            const int d = row / (D + 1), e = row - d * (D + 1), d2 = col / (D + 1), e2 = col - d2 * (D + 1);
            const int k = pair_index(d < d2 ? d : d2, d < d2 ? d2 : d, D);
            const int m = pair_index(e < e2 ? e : e2, e < e2 ? e2 : e, D + 1);
            hessian[b * P * P + t] = (R)tot[1 + P + k * M + m];
        }
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------
// Validate + convert: vol_* is moving as interpol_pull takes its vol, grid_shape the lattice, val_* is fixed as interpol_pull takes
// its val.  *mspan: the bytes one (batch, channel) image of moving spans.
static int sa_params(const interpol_problem *p, KParams *k, int *B, uint64_t *mspan)
{
    if (!p) return INTERPOL_E_NULL;
    if (p->abi_version != INTERPOL_ABI_VERSION) return INTERPOL_E_SHAPE;
    if (p->dim < 1 || p->dim > 3) return INTERPOL_E_DIM;
    if (p->extrapolate < 0 || p->extrapolate > 2) return INTERPOL_E_EXTRAP;
    if (p->dtype != INTERPOL_F32 && p->dtype != INTERPOL_F64) return INTERPOL_E_DTYPE;
    if (p->grid_dtype != p->dtype) return INTERPOL_E_DTYPE;
    if (p->batch < 1 || p->batch > 65535 || p->channels < 1 || p->channels > 0x7fffffff) return INTERPOL_E_SHAPE;   // (the item is on gridDim.y)
    if (p->flags & (INTERPOL_FLAG_SEPARABLE_GRID | INTERPOL_FLAG_DISPLACEMENT)) return INTERPOL_E_STRIDE;   // the lattice is affine
    const int D = p->dim;
    const uint64_t es = p->dtype == INTERPOL_F64 ? 8 : 4;
    memset(k, 0, sizeof(*k));
    k->dim = D;
    k->extrapolate = p->extrapolate;
    for (int d = 0; d < D; ++d) {
        if (p->order[d] < 0 || p->order[d] > 7) return INTERPOL_E_ORDER;
        if (p->bound[d] < 0 || p->bound[d] > 6) return INTERPOL_E_BOUND;
        if (p->vol_shape[d] < 1 || p->vol_shape[d] > 0x3fffffff) return INTERPOL_E_SHAPE;
        if (p->grid_shape[d] < 1 || p->grid_shape[d] > 0x7fffffffll) return INTERPOL_E_SHAPE;
    }
    for (int d = 0; d < D; ++d)
        if (p->order[d] != p->order[0] || p->order[0] < 1 || p->order[0] > 3) return INTERPOL_E_ORDER;   // one order 1..3
    // moving: any non-negative strides, one image within 32-bit byte offsets
    uint64_t max_off = 0;
    for (int d = 0; d < D; ++d) {
        if (p->vol_stride[2 + d] < 0) return INTERPOL_E_STRIDE;
        const uint64_t sbytes = (uint64_t)p->vol_stride[2 + d] * es;
        if (sbytes > 0x7fffffffull) return INTERPOL_E_STRIDE;
        k->vol_ss[d] = (int)sbytes;
        max_off += (uint64_t)(p->vol_shape[d] - 1) * sbytes;
    }
    if (max_off + es > 0xffffffffull) return INTERPOL_E_SHAPE;      // one item of a gather source spans < 4 GiB
    *mspan = max_off + es;
    // fixed: row-major over the sample lattice
    int64_t fexp = 1, N = 1;
    for (int d = D - 1; d >= 0; --d) {
        if (p->grid_shape[d] > 1 && p->val_stride[2 + d] != fexp) return INTERPOL_E_STRIDE;
        fexp *= p->grid_shape[d];
        N *= p->grid_shape[d];
        if (N > 0xffffffffll) return INTERPOL_E_SHAPE;              // the sample index is split in 32 bits (load_coords)
    }
    if (p->vol_stride[0] < 0 || p->vol_stride[1] < 0 || p->val_stride[0] < 0 || p->val_stride[1] < 0) return INTERPOL_E_STRIDE;
    bool all1 = true;
    for (int d = 0; d < 3; ++d) {
        if (d >= D) { k->bound[d] = 1; k->order[d] = 0; k->vol_n[d] = 1; k->vol_ss[d] = 0; k->gshape[d] = 1; continue; }
        k->bound[d] = p->bound[d];
        k->order[d] = p->order[d];
        k->vol_n[d] = (int)p->vol_shape[d];
        k->gshape[d] = (int)p->grid_shape[d];
        all1 = all1 && p->order[d] == 1;
        k->mask_hi[d] = (double)(p->vol_shape[d] - 1) + (p->extrapolate == 2 ? 0.5 + 5e-2 : 5e-2);
    }
    k->mask_lo = -(p->extrapolate == 2 ? 0.5 + 5e-2 : 5e-2);
    k->mask_lo_f = (float)k->mask_lo;
    for (int d = 0; d < 3; ++d) k->mask_hi_f[d] = (float)k->mask_hi[d];
    k->mode = all1 ? MODE_ISO1 : MODE_ND;                           // pushpull.py:48-66
    k->C = (int)p->channels;
    k->sep = 3;                                                     // x = A o + t from the matrix (load_coords)
    k->N = N;
    k->vol_sb = p->vol_stride[0];
    k->vol_sc = p->vol_stride[1];
    k->val_sb = p->val_stride[0];
    k->val_sc = p->val_stride[1];
    *B = (int)p->batch;
    return 0;
}

// the bytes of the sums of the call WITH a Hessian: a function of the problem alone
static int64_t sa_workspace(int D, int B) { return (int64_t)B * num_sums(D, true) * SA_BLOCKS * (int64_t)sizeof(double); }

} // namespace ssd_affine
} // namespace ip
