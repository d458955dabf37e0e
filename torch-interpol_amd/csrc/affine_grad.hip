// ===========================================================================
// affine_grad.hip -- gradient of the matrix of an affine lattice (INTERPOL_FLAG_AFFINE_GRID).
//
// With x(o) = A o + t evaluated in registers (stencil.hpp: load_coords, sep == 3) the chain rule through
// affine_grid (reference interpol/api.py:534-572) contracts the per-sample grid gradient g(b, o) of
// grid_pull_backward / grid_push_backward / grid_count_backward (reference pushpull.py:237-299) with the
// sample index:
//     dL/dA[d,e] = sum_b sum_o g_d(b,o) * o_e          dL/dt[d] = sum_b sum_o g_d(b,o)
// g is computed per sample exactly as pullbwd_generic / pushbwd_generic (ops_generic.hpp) compute their
// gg0..gg2 -- same load_coords, Stencil<NEED_G>, mask, channel loop and operation order -- and is never
// stored: nothing of size N touches memory but the images.
//
// Reduction, without atomics and in a fixed order (bit-identical from run to run):
//   affine_grad_partial : AG_BLOCKS persistent workgroups (a constant: the summation tree does not depend on the
//       shape) stride over the samples; every thread keeps the D (D+1) sums in DOUBLE whatever the image dtype
//       (the products g_d * o_e are exact in double: 24 or 53 bits times an integer below 2^32 rounds once, at
//       the add); wave reduction by shuffles, workgroup reduction through LDS, one row of D (D+1) doubles per
//       workgroup into the workspace (every workgroup writes its row: the workspace need not be cleared);
//   affine_grad_finish  : one workgroup sums the rows the same way and writes grad_mat in the grid dtype.
//
// Compiled once per storage type, with the macros of ops_instantiate.inc (IP_T, IP_G, IP_R, IP_SFX), and
// dispatched over (D, order, ISO) by launch.hpp like the generic kernels.
// ===========================================================================
#include "ops_generic.hpp"
#include "launch.hpp"
#include "route.hpp"
#include "affine_grad.hpp"

namespace ip {

// sum of `acc[i]` over the workgroup, for every i < NA, in a fixed order: lanes by halving shuffles, then the waves
// one after the other.  Valid in threads i < NA on return.
template <int NA>
__device__ __forceinline__ void block_sum(double (&acc)[NA], double (*part)[NA])
{
#pragma unroll
    for (int i = 0; i < NA; ++i) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc[i] += __shfl_down(acc[i], off, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NA; ++i) part[wave][i] = acc[i];
    }
    __syncthreads();
    if (threadIdx.x < NA) {
        double s = part[0][threadIdx.x];
        for (int w = 1; w < BLOCK / 64; ++w) s += part[w][threadIdx.x];
        acc[0] = s;
    }
}

// src: grad_out of the pull (pushpull.py:237-258) or val of the push (262-282), (B, C, *grid_shape) through p.val_sb /
// p.val_sc; COUNT: all ones (286-299).  vol: the image the stencil indexes (vol of the pull, grad_vol_out of the push).
template <typename T, typename G, typename R, int D, int KMAX, bool ISO, bool COUNT>
__global__ __launch_bounds__(BLOCK) void affine_grad_partial(KParams p, const T *__restrict__ src, const T *__restrict__ vol,
                                                             const G *__restrict__ mat, double *__restrict__ rows, int B)
{
    constexpr int NA = D * (D + 1);
    __shared__ double part[BLOCK / 64][NA];
    double acc[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) acc[i] = 0.0;
    const int64_t step = (int64_t)gridDim.x * BLOCK;
    for (int64_t b = 0; b < B; ++b) {
        const T *vb = vol + b * p.vol_sb;
        for (int64_t o = (int64_t)blockIdx.x * BLOCK + threadIdx.x; o < p.N; o += step) {
            R x[D];
            load_coords<R, G, D>(p, mat, b, o, x);
            Stencil<R, D, KMAX, ISO, NEED_G> s;
            s.setup(p, x);
            R gg0 = R(0), gg1 = R(0), gg2 = R(0);
            for (int c = 0; c < p.C; ++c) {
                const T *v0 = vb + c * p.vol_sc;
                R sv = s.mask;
                if (!COUNT) sv *= Cvt<R, T>::ld(src[b * p.val_sb + c * p.val_sc + o]);
                opaque(s);
                R a0 = R(0), a1 = R(0), a2 = R(0);
                IP_FOR_I {
                    R pWW = R(0), pGW = R(0), pWG = R(0);
                    IP_FOR_J {
                        const unsigned oij = s.off[0][i] + s.off[1][j];
                        R rW = R(0), rG = R(0);
                        IP_FOR_K {
                            const R v = Cvt<R, T>::ld(ld_tap(v0, oij + s.off[2][k]));
                            rW = fma_(s.w[2][k], v, rW);
                            if (D > 2) rG = fma_(s.g[2][k], v, rG);
                        } IP_ROW_END;
                        pWW = fma_(s.w[1][j], rW, pWW);
                        if (D > 1) pGW = fma_(s.g[1][j], rW, pGW);
                        if (D > 2) pWG = fma_(s.w[1][j], rG, pWG);
                    }
                    a0 = fma_(s.g[0][i], pWW, a0);
                    if (D > 1) a1 = fma_(s.w[0][i], pGW, a1);
                    if (D > 2) a2 = fma_(s.w[0][i], pWG, a2);
                }
                gg0 = fma_(a0, sv, gg0); gg1 = fma_(a1, sv, gg1); gg2 = fma_(a2, sv, gg2);
            }
            // the integer index of the sample (the split of load_coords), and the per-sample gradient as the generic kernels
            // store it (rounded to the grid dtype); one conversion to double each, at the accumulate
            unsigned r = (unsigned)o;
            double od[D + 1];
#pragma unroll
            for (int d = D - 1; d > 0; --d) { const unsigned q = r / (unsigned)p.gshape[d]; od[d] = (double)(r - q * (unsigned)p.gshape[d]); r = q; }
            od[0] = (double)r;
            od[D] = 1.0;
            const double g[3] = { (double)(G)gg0, (double)(G)gg1, (double)(G)gg2 };
#pragma unroll
            for (int d = 0; d < D; ++d) {
#pragma unroll
                for (int e = 0; e <= D; ++e) acc[d * (D + 1) + e] = __builtin_fma(g[d], od[e], acc[d * (D + 1) + e]);
            }
        }
    }
    block_sum<NA>(acc, part);
    if (threadIdx.x < NA) rows[(int64_t)blockIdx.x * NA + threadIdx.x] = acc[0];
}

// (T only keeps the symbols of the translation units apart: bf16 / f16 / f32 share G = float)
template <typename T, typename G, int NA>
__global__ __launch_bounds__(BLOCK) void affine_grad_finish(const double *__restrict__ rows, int nrows, G *__restrict__ grad_mat)
{
    __shared__ double part[BLOCK / 64][NA];
    double acc[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) acc[i] = 0.0;
    for (int r = threadIdx.x; r < nrows; r += BLOCK) {
#pragma unroll
        for (int i = 0; i < NA; ++i) acc[i] += rows[(int64_t)r * NA + i];
    }
    block_sum<NA>(acc, part);
    if (threadIdx.x < NA) grad_mat[threadIdx.x] = (G)acc[0];
}

#define IP_NAME2(a, b) a##b
#define IP_NAME(a, b) IP_NAME2(a, b)

// src == NULL: count.  rows: affine_grad_workspace_bytes(p.dim) bytes.  0, or what dispatch_variant returns.
int IP_NAME(launch_affine_grad_, IP_SFX)(const KParams &p, const void *src, const void *vol, const void *mat, void *rows,
                                         void *grad_mat, int B, hipStream_t st)
{
    return dispatch_variant(p, [&](auto d, auto k, auto iso) {
        constexpr int D = decltype(d)::value; constexpr int K = decltype(k)::value; constexpr bool I = decltype(iso)::value;
        if (src)
            hipLaunchKernelGGL((affine_grad_partial<IP_T, IP_G, IP_R, D, K, I, false>), dim3(AG_BLOCKS), dim3(BLOCK), 0, st,
                               p, (const IP_T *)src, (const IP_T *)vol, (const IP_G *)mat, (double *)rows, B);
        else
            hipLaunchKernelGGL((affine_grad_partial<IP_T, IP_G, IP_R, D, K, I, true>), dim3(AG_BLOCKS), dim3(BLOCK), 0, st,
                               p, (const IP_T *)nullptr, (const IP_T *)vol, (const IP_G *)mat, (double *)rows, B);
        hipLaunchKernelGGL((affine_grad_finish<IP_T, IP_G, D * (D + 1)>), dim3(1), dim3(BLOCK), 0, st,
                           (const double *)rows, AG_BLOCKS, (IP_G *)grad_mat);
    });
}

} // namespace ip
