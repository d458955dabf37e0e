// ===========================================================================
// ssd_affine.hip -- the sum-of-squares data term of a Gauss-Newton step on the matrix of an AFFINE lattice: loss, gradient of
// the D (D+1) matrix entries and their P x P Gauss-Newton Hessian (P = D (D+1)) in one pass over the samples.
//
//     x(o)    = A_b o + t_b                                      load_coords, sep == 3, from mat + b * stride (one matrix per item)
//     w_c(o)  = mask(x) sum_taps W(x) sign moving[b, c, wrap(tap)]                                          (= grid_pull)
//     G_cd(o) = mask(x) sum_taps dW/dx_d(x) sign moving[b, c, wrap(tap)]                                    (= grid_grad)
//     r_c     = w_c - fixed[b, c, o],        o~ = (o_0 .. o_{D-1}, 1)
//     loss[b]                               = 1/2 sum_o weight sum_c r_c^2
//     gradient[b, d, e]                     = sum_o (weight sum_c r_c G_cd) o~_e
//     hessian[b, d (D+1) + e, d' (D+1) + e'] = sum_o (weight sum_c G_cd G_cd') o~_e o~_e'
//
// Nothing of size N touches memory but the two images (and the weight): no lattice, no per-sample gradient or Hessian field.
//
//   ssd_affine_partial<R, D, KMAX, HESS> : SA_BLOCKS persistent workgroups per batch item (a CONSTANT: the summation tree depends
//       on the shape alone), the item on gridDim.y.  A workgroup takes runs of BLOCK consecutive samples, SA_BLOCKS runs apart.
//       Per sample: the affine branch of load_coords, ONE Stencil<R, D, K, true, NEED_G> for every channel and the channel loop of
//       ssd_fwd (ssd.hip).  In R: the loss term weight sum_c r_c^2, q_d = weight sum_c r_c G_cd and h_dd' = weight sum_c G_cd
//       G_cd' (d <= d'); each is converted to double ONCE and multiplied into the NS sums held in double in registers:
//           [0]                         the loss term
//           [1 + d (D+1) + e]           q_d o~_e
//           [1 + P + pair(d,d') M + pair(e,e')]   h_dd' o~_e o~_e',   M = (D+1)(D+2)/2 moments, pair: upper triangle row by row
//       NS = 1 + P + D(D+1)/2 * M: 73 / 25 / 6 for D = 3 / 2 / 1; without a Hessian 1 + P.  (o~_e o~_e' is exact in double whenever
//       it is below 2^53.)  One fixed-order workgroup reduction at the end (lanes by halving shuffles, then the waves in turn);
//       every workgroup writes its NS doubles, also when it met no sample: workspace[b][i][workgroup].
//   ssd_affine_partial_staged<R, D, KMAX> : the same sums with ONE accumulator per thread, the per-sample terms staged through LDS;
//       serves 3-D cubic with a Hessian, where it was measured faster (see `staged`).  Same workspace, same finish.
//   ssd_affine_finish<R, D, HESS>        : one workgroup per item; wave w sums the SA_BLOCKS doubles of the sums i = w, w + 4, ..:
//       16 independent partial sums per lane, folded in a fixed order, then the lanes by halving shuffles.  Writes the loss, the
//       gradient and BOTH triangles of the Hessian (from the same sum: exactly symmetric) in R.
//
// No atomics, nothing in the workspace is assumed cleared: two calls give identical bits, an item gives the same bits alone or
// inside a batch, and the two launches replay from a captured graph to the bits of eager.
// `weight` is a nullable pointer (block-uniform branch).  Instantiated for float / double, D = 1..3, one order 1..3 in every dim,
// with and without the Hessian.  The C entry points live here as well (include/interpol_hip.h: interpol_ssd_affine_workspace,
// interpol_ssd_affine).
// ===========================================================================
#include "../../include/interpol_hip.h"
#include "regulariser_at.hpp"                                      // ops_generic.hpp, ranges_overlap
#include <hip/hip_runtime.h>
#include <string.h>

namespace ip {
namespace ssd_affine {

// Persistent workgroups of ssd_affine_partial per batch item = doubles per sum and item in the workspace.  A CONSTANT.
constexpr int SA_BLOCKS = 1024;
constexpr int WAVES = BLOCK / 64;
constexpr int FINISH_WAYS = SA_BLOCKS / 64;                         // the doubles of one sum that one lane of ssd_affine_finish adds

constexpr int params(int D) { return D * (D + 1); }
constexpr int moments(int D) { return (D + 1) * (D + 2) / 2; }
constexpr int num_sums(int D, bool hess) { return 1 + params(D) + (hess ? (D * (D + 1) / 2) * moments(D) : 0); }
// index of (i, j), i <= j < n, in the upper triangle of an n x n matrix, row by row
__host__ __device__ constexpr int pair_index(int i, int j, int n) { return i * n - i * (i - 1) / 2 + (j - i); }

// The terms of sample o, formed in R: the coordinate by the affine branch of load_coords from `ab`, one stencil for every channel and
// the channel loop of ssd_fwd.  lt = weight sum_c r_c^2, q[d] = weight sum_c r_c G_cd, h[pair(d, d')] = weight sum_c G_cd G_cd'
// (HESS), od = (o_0 .. o_{D-1}, 1) as doubles (the split of load_coords).
template <typename R, int D, int KMAX, bool HESS>
__device__ __forceinline__ void sample_terms(const KParams &p, const R *mb, const R *fb, const R *ab, const R *wb, int64_t o,
                                             double *od, R &lt, R *q, R *h)
{
    constexpr int K = D * (D + 1) / 2;
    R x[D];
    load_coords<R, R, D>(p, ab, 0, o, x);
    Stencil<R, D, KMAX, true, NEED_G> s;
    s.setup(p, x);
    const R wt = wb ? wb[o] : R(1);
    R ga[D], ha[K], la = R(0);
#pragma unroll
    for (int d = 0; d < D; ++d) ga[d] = R(0);
#pragma unroll
    for (int k = 0; k < K; ++k) ha[k] = R(0);
    for (int c = 0; c < p.C; ++c) {
        const R *v0 = mb + c * p.vol_sc;
        opaque(s);
        R a0 = R(0), a1 = R(0), a2 = R(0), aw = R(0);
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
        const R av[3] = { a0, a1, a2 };
        R g[D];
#pragma unroll
        for (int d = 0; d < D; ++d) g[d] = av[d] * s.mask;
        const R r = aw * s.mask - fb[c * p.val_sc + o];
        la = fma_(r, r, la);
#pragma unroll
        for (int d = 0; d < D; ++d) ga[d] = fma_(r, g[d], ga[d]);
        if (HESS) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
#pragma unroll
                for (int e = d; e < D; ++e) ha[pair_index(d, e, D)] = fma_(g[d], g[e], ha[pair_index(d, e, D)]);
            }
        }
    }
    unsigned rr = (unsigned)o;
#pragma unroll
    for (int d = D - 1; d > 0; --d) { const unsigned qq = rr / (unsigned)p.gshape[d]; od[d] = (double)(rr - qq * (unsigned)p.gshape[d]); rr = qq; }
    od[0] = (double)rr;
    od[D] = 1.0;
    lt = wt * la;
#pragma unroll
    for (int d = 0; d < D; ++d) q[d] = wt * ga[d];
    if (HESS) {
#pragma unroll
        for (int k = 0; k < K; ++k) h[k] = wt * ha[k];
    }
}

// moving (B, C, *in) through p.vol_sb / p.vol_sc / p.vol_ss (bytes), fixed (B, C, *shape) through p.val_sb / p.val_sc, mat
// (B, D, D+1) through mat_sb, weight (B, *shape) through weight_sb; sums (B, NS, SA_BLOCKS) doubles
template <typename R, int D, int KMAX, bool HESS>
__global__ __launch_bounds__(BLOCK) void ssd_affine_partial(KParams p, const R *__restrict__ moving, const R *__restrict__ fixed,
                                                            const R *__restrict__ mat, const R *__restrict__ weight,
                                                            double *__restrict__ sums, int64_t mat_sb, int64_t weight_sb)
{
    constexpr int P = params(D), M = moments(D), NS = num_sums(D, HESS), K = D * (D + 1) / 2;
    __shared__ double part[WAVES][NS];
    const int64_t b = blockIdx.y;
    const R *mb = moving + b * p.vol_sb;
    const R *fb = fixed + b * p.val_sb;
    const R *ab = mat + b * mat_sb;
    const R *wb = weight ? weight + b * weight_sb : nullptr;
    double acc[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) acc[i] = 0.0;
    for (int64_t o = (int64_t)blockIdx.x * BLOCK + threadIdx.x; o < p.N; o += (int64_t)SA_BLOCKS * BLOCK) {
        double od[D + 1];
        R lt, q[D], h[K];
        sample_terms<R, D, KMAX, HESS>(p, mb, fb, ab, wb, o, od, lt, q, h);
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
// 219 of the 256 threads add).  The parts are added in turn at the end.  Which organisation serves which order: `staged` below.
template <typename R, int D, int KMAX>
__global__ __launch_bounds__(BLOCK) void ssd_affine_partial_staged(KParams p, const R *__restrict__ moving, const R *__restrict__ fixed,
                                                                   const R *__restrict__ mat, const R *__restrict__ weight,
                                                                   double *__restrict__ sums, int64_t mat_sb, int64_t weight_sb)
{
    constexpr int P = params(D), M = moments(D), NS = num_sums(D, true), K = D * (D + 1) / 2;
    constexpr int NV = 1 + D + K, REC = NV + D + 1, GROUPS = BLOCK / NS, PER = (BLOCK + GROUPS - 1) / GROUPS;
    static_assert(GROUPS >= 1, "one thread per sum at least");
    __shared__ double stage[BLOCK * REC];
    __shared__ double part[GROUPS][NS];
    const int64_t b = blockIdx.y;
    const R *mb = moving + b * p.vol_sb;
    const R *fb = fixed + b * p.val_sb;
    const R *ab = mat + b * mat_sb;
    const R *wb = weight ? weight + b * weight_sb : nullptr;
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
            sample_terms<R, D, KMAX, true>(p, mb, fb, ab, wb, o, od, lt, q, h);
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

// Measured at 1 x 1 x 256^3 and 4 x 2 x 256^3 float32 (profiles/ssd_affine.txt): the staged sums win where the stencil is large
// (cubic: 1.24 against 1.56 ms, 7.3 against 9.6 ms) and lose where it is small (linear 0.67 against 0.63 ms, quadratic 0.90 against
// 0.84 ms: the LDS pass costs more than the occupancy brings).
constexpr bool staged(int D, int KMAX, bool hess) { return hess && D == 3 && KMAX == 3; }

// sums (B, NS, SA_BLOCKS) doubles -> loss (B), gradient (B, D, D+1), hessian (B, P, P)
template <typename R, int D, bool HESS>
__global__ __launch_bounds__(BLOCK) void ssd_affine_finish(const double *__restrict__ sums, R *__restrict__ loss,
                                                           R *__restrict__ gradient, R *__restrict__ hessian)
{
    constexpr int P = params(D), M = moments(D), NS = num_sums(D, HESS);
    __shared__ double tot[NS];
    const int64_t b = blockIdx.x;
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
    if (threadIdx.x == 0) loss[b] = (R)(0.5 * tot[0]);
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

struct Args {
    KParams k; int B; bool hess; int64_t mat_sb, weight_sb;
    const void *moving, *fixed, *mat, *weight; void *loss, *gradient, *hessian; double *sums; hipStream_t st;
};

template <typename R, int D, int KMAX, bool HESS>
static void sa_launch(const Args &a)
{
    if constexpr (staged(D, KMAX, HESS))
        hipLaunchKernelGGL((ssd_affine_partial_staged<R, D, KMAX>), dim3(SA_BLOCKS, (unsigned)a.B, 1), dim3(BLOCK), 0, a.st, a.k,
                           (const R *)a.moving, (const R *)a.fixed, (const R *)a.mat, (const R *)a.weight, a.sums, a.mat_sb, a.weight_sb);
    else
        hipLaunchKernelGGL((ssd_affine_partial<R, D, KMAX, HESS>), dim3(SA_BLOCKS, (unsigned)a.B, 1), dim3(BLOCK), 0, a.st, a.k,
                           (const R *)a.moving, (const R *)a.fixed, (const R *)a.mat, (const R *)a.weight, a.sums, a.mat_sb, a.weight_sb);
    hipLaunchKernelGGL((ssd_affine_finish<R, D, HESS>), dim3((unsigned)a.B), dim3(BLOCK), 0, a.st, (const double *)a.sums,
                       (R *)a.loss, (R *)a.gradient, (R *)a.hessian);
}

template <typename R, int D, int KMAX>
static void sa_by_hessian(const Args &a)
{
    if (a.hess) sa_launch<R, D, KMAX, true>(a);
    else sa_launch<R, D, KMAX, false>(a);
}

template <typename R, int D>
static void sa_by_order(const Args &a)
{
    switch (a.k.order[0]) {
    case 1: return sa_by_hessian<R, D, 1>(a);
    case 2: return sa_by_hessian<R, D, 2>(a);
    default: return sa_by_hessian<R, D, 3>(a);
    }
}

template <typename R>
static void sa_by_dim(const Args &a)
{
    switch (a.k.dim) {
    case 1: return sa_by_order<R, 1>(a);
    case 2: return sa_by_order<R, 2>(a);
    default: return sa_by_order<R, 3>(a);
    }
}

// the workspace holds the sums of the call WITH a Hessian: a function of the problem alone
static int64_t sa_workspace(int D, int B) { return (int64_t)B * num_sums(D, true) * SA_BLOCKS * (int64_t)sizeof(double); }

} // namespace ssd_affine
} // namespace ip

extern "C" {

int64_t interpol_ssd_affine_workspace(const interpol_problem *p)
{
    ip::KParams k; int B; uint64_t mspan;
    const int rc = ip::ssd_affine::sa_params(p, &k, &B, &mspan);
    if (rc) return rc;
    return ip::ssd_affine::sa_workspace(k.dim, B);
}

int interpol_ssd_affine(const interpol_problem *p, const void *moving, const void *fixed, const void *mat, const void *weight,
                        void *loss, void *gradient, void *hessian, int with_hessian, int64_t mat_batch_stride,
                        int64_t weight_batch_stride, void *workspace, int64_t workspace_bytes, void *stream)
{
    using namespace ip::ssd_affine;
    using ip::reg::ranges_overlap;
    Args a;
    uint64_t mimage;
    const int rc = sa_params(p, &a.k, &a.B, &mimage);
    if (rc) return rc;
    if (with_hessian != 0 && with_hessian != 1) return INTERPOL_E_SHAPE;
    a.hess = with_hessian != 0;
    const int D = a.k.dim;
    const uint64_t B = (uint64_t)a.B, N = (uint64_t)a.k.N, C = (uint64_t)a.k.C, P = (uint64_t)params(D);
    const uint64_t es = p->dtype == INTERPOL_F64 ? 8 : 4;
    if (mat_batch_stride < 0 || (weight && weight_batch_stride < 0)) return INTERPOL_E_STRIDE;
    if (!moving || !fixed || !mat || !loss || !gradient || !workspace || (a.hess && !hessian)) return INTERPOL_E_NULL;
    if ((uintptr_t)workspace % sizeof(double)) return INTERPOL_E_STRIDE;             // (the sums are doubles)
    const uint64_t wsbytes = (uint64_t)sa_workspace(D, a.B);
    if (workspace_bytes < (int64_t)wsbytes) return INTERPOL_E_SCRATCH;
    // what is written (loss, gradient, hessian, workspace) overlaps neither an input nor each other
    const void *rd[4] = { moving, fixed, mat, weight };
    const uint64_t rn[4] = { ((B - 1) * (uint64_t)a.k.vol_sb + (C - 1) * (uint64_t)a.k.vol_sc) * es + mimage,
                             ((B - 1) * (uint64_t)a.k.val_sb + (C - 1) * (uint64_t)a.k.val_sc + N) * es,
                             ((B - 1) * (uint64_t)mat_batch_stride + P) * es,
                             weight ? ((B - 1) * (uint64_t)weight_batch_stride + N) * es : 0 };
    const void *wr[4] = { loss, gradient, hessian, workspace };
    const uint64_t wn[4] = { B * es, B * P * es, a.hess ? B * P * P * es : 0, wsbytes };
    for (int i = 0; i < 4; ++i) {
        if (!wn[i]) continue;
        for (int j = 0; j < 4; ++j)
            if (rn[j] && ranges_overlap(wr[i], wn[i], rd[j], rn[j])) return INTERPOL_E_STRIDE;
        for (int j = i + 1; j < 4; ++j)
            if (wn[j] && ranges_overlap(wr[i], wn[i], wr[j], wn[j])) return INTERPOL_E_STRIDE;
    }
    a.mat_sb = mat_batch_stride;
    a.weight_sb = weight ? weight_batch_stride : 0;
    a.moving = moving; a.fixed = fixed; a.mat = mat; a.weight = weight;
    a.loss = loss; a.gradient = gradient; a.hessian = a.hess ? hessian : nullptr;
    a.sums = (double *)workspace; a.st = (hipStream_t)stream;
    if (p->dtype == INTERPOL_F64) sa_by_dim<double>(a);
    else sa_by_dim<float>(a);
    return hipGetLastError() == hipSuccess ? 0 : INTERPOL_E_LAUNCH;
}

} // extern "C"
