// ===========================================================================
// regulariser_solve.hpp -- what the two solvers of (H + L) x = g share (regulariser_solve.hip: conjugate gradients with the
// per-point preconditioner; regulariser_multigrid.hip: the same conjugate gradients with a V-cycle as preconditioner): the
// per-point Hessian helpers and the closed-form inverse of M_o = H_o + diag(c), the runs of the reducing kernels, the
// direction update, the per-item scalars, and the host-side pieces of the validation.
// ===========================================================================
#pragma once
#include "regulariser_at.hpp"

namespace ip {
namespace reg {

enum { HK_NONE = 0, HK_DIAG = 1, HK_FULL = 2 };
// the scalars of one item (doubles)
enum { S_RHO = 0, S_GAMMA, S_ALPHA, S_BETA, S_SIGMA, S_ITER, S_DONE, S_STRIDE = 8 };

template <typename R> struct Diag { R c[3]; };

constexpr int hess_count(int D, int HK) { return HK == HK_NONE ? 0 : (HK == HK_DIAG ? D : D * (D + 1) / 2); }

// h[0..K): the Hessian of one lattice point (K components of R, aligned like one component)
template <typename R, int K>
__device__ __forceinline__ void load_hess(const R *hb, int64_t o, R (&h)[6])
{
    if constexpr (K > 0) {
        const PointVec<R, K> v = *reinterpret_cast<const PointVec<R, K> *>(hb + o * K);
#pragma unroll
        for (int i = 0; i < K; ++i) h[i] = v.c[i];
    }
}

// z = (H_o + diag(c))^-1 r in closed form (the adjugate of the symmetric matrix over its determinant)
template <typename R, int D, int HK>
__device__ __forceinline__ void precond(const R (&h)[6], const Diag<R> &c, const R (&r)[D], R (&z)[D])
{
    R m[D];
#pragma unroll
    for (int d = 0; d < D; ++d) m[d] = HK == HK_NONE ? c.c[d] : h[d] + c.c[d];
    if constexpr (HK != HK_FULL || D == 1) {
#pragma unroll
        for (int d = 0; d < D; ++d) z[d] = r[d] / m[d];
    } else if constexpr (D == 2) {
        const R b = h[2];
        const R inv = R(1) / (m[0] * m[1] - b * b);
        z[0] = (m[1] * r[0] - b * r[1]) * inv;
        z[1] = (m[0] * r[1] - b * r[0]) * inv;
    } else {
        const R a01 = h[3], a02 = h[4], a12 = h[5];
        const R c00 = m[1] * m[2] - a12 * a12, c01 = a02 * a12 - a01 * m[2], c02 = a01 * a12 - a02 * m[1];
        const R c11 = m[0] * m[2] - a02 * a02, c12 = a01 * a02 - m[0] * a12, c22 = m[0] * m[1] - a01 * a01;
        const R inv = R(1) / (m[0] * c00 + a01 * c01 + a02 * c02);
        z[0] = (c00 * r[0] + c01 * r[1] + c02 * r[2]) * inv;
        z[1] = (c01 * r[0] + c11 * r[1] + c12 * r[2]) * inv;
        z[2] = (c02 * r[0] + c12 * r[1] + c22 * r[2]) * inv;
    }
}

// q += H_o v
template <typename R, int D, int HK>
__device__ __forceinline__ void hess_mul(const R (&h)[6], const R (&v)[D], R (&q)[D])
{
    if constexpr (HK == HK_DIAG || (HK == HK_FULL && D == 1)) {
#pragma unroll
        for (int d = 0; d < D; ++d) q[d] = fma_(h[d], v[d], q[d]);
    } else if constexpr (HK == HK_FULL && D == 2) {
        q[0] += fma_(h[0], v[0], h[2] * v[1]);
        q[1] += fma_(h[2], v[0], h[1] * v[1]);
    } else if constexpr (HK == HK_FULL && D == 3) {
        q[0] += fma_(h[0], v[0], fma_(h[3], v[1], h[4] * v[2]));
        q[1] += fma_(h[3], v[0], fma_(h[1], v[1], h[5] * v[2]));
        q[2] += fma_(h[4], v[0], fma_(h[5], v[1], h[2] * v[2]));
    }
}

// the run of consecutive points of workgroup `g` (whole multiples of BLOCK; reg_energy's)
__device__ __forceinline__ void run_of(int64_t N, int g, int64_t &lo, int64_t &hi)
{
    const int64_t chunk = ((N + RG_BLOCKS - 1) / RG_BLOCKS + BLOCK - 1) / BLOCK * BLOCK;
    lo = g * chunk;
    hi = lo + chunk < N ? lo + chunk : N;
}

// p = z + beta p over the n = N D elements of every item that is not done
template <typename R>
__global__ __launch_bounds__(BLOCK) void solve_direction(int64_t n, const R *__restrict__ z, R *__restrict__ pp, const double *__restrict__ scal, int B)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        if (scal[b * S_STRIDE + S_DONE] != 0.0) continue;
        const R beta = (R)scal[b * S_STRIDE + S_BETA];
        pp[b * n + i] = fma_(beta, pp[b * n + i], z[b * n + i]);
    }
}

// PHASE 0: after solve_init; 1: after solve_matvec; 2: after solve_update.  One workgroup per item; info (B, 2) doubles or NULL
template <int PHASE>
__global__ __launch_bounds__(BLOCK) void solve_scalars(const double *__restrict__ slots, double *scal, double *info, double tol2, int B)
{
    __shared__ double part[BLOCK / 64];
    for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
        double *s = scal + b * S_STRIDE;
        // (read by every thread before thread 0 writes it behind the barriers of block_sum1: uniform)
        if (PHASE != 0 && s[S_DONE] != 0.0) continue;
        double acc0 = 0.0, acc1 = 0.0;
        for (int r = threadIdx.x; r < RG_BLOCKS; r += BLOCK) {
            acc0 += slots[(b * RG_BLOCKS + r) * 2];
            if (PHASE != 1) acc1 += slots[(b * RG_BLOCKS + r) * 2 + 1];
        }
        const double s0 = block_sum1(acc0, part);
        const double s1 = PHASE != 1 ? block_sum1(acc1, part) : 0.0;
        if (threadIdx.x != 0) continue;
        if (PHASE == 0) {
            s[S_RHO] = s0; s[S_GAMMA] = s1; s[S_ALPHA] = 0.0; s[S_BETA] = 0.0; s[S_SIGMA] = 0.0; s[S_ITER] = 0.0;
            s[S_DONE] = s1 == 0.0 ? 1.0 : 0.0;
            s[S_STRIDE - 1] = 0.0;
            if (info) { info[2 * b] = 0.0; info[2 * b + 1] = 0.0; }
        } else if (PHASE == 1) {
            const double rho = s[S_RHO];
            if (s0 <= 0.0 || rho <= 0.0) s[S_DONE] = 1.0;
            else s[S_ALPHA] = rho / s0;
        } else {
            const double it = s[S_ITER] + 1.0, gamma = s[S_GAMMA];
            s[S_ITER] = it;
            s[S_SIGMA] = s1;
            if (info) { info[2 * b] = it; info[2 * b + 1] = sqrt(s1 / gamma); }
            if (s1 <= tol2 * gamma) s[S_DONE] = 1.0;
            else { s[S_BETA] = s0 / s[S_RHO]; s[S_RHO] = s0; }
        }
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------
static int64_t align256(int64_t v) { return (v + 255) / 256 * 256; }

// the mode (none / diagonal / full) of `components` Hessian entries per point, or INTERPOL_E_SHAPE
static int hess_kind(int D, int components)
{
    if (components == 0) return HK_NONE;
    if (components == D) return HK_DIAG;                            // (D = 1: the diagonal is the matrix)
    if (components == D * (D + 1) / 2) return HK_FULL;
    return INTERPOL_E_SHAPE;
}

// the problem alone: the field, the bounds under which the three terms are symmetric (slide: as reg_params)
static int solve_params(const interpol_problem *p, KParams *k, int *B, int *slide = nullptr)
{
    const int rc = reg_params(p, false, k, B, slide);
    if (rc) return rc;
    return reg_symmetric(*k, slide ? *slide : 0, false) ? 0 : INTERPOL_E_BOUND;
}

// c_d = h_d^2 [ absolute + membrane sum_e 2 / h_e^2 + bending ( sum_e 6 / h_e^4 + sum_{e != f} 4 / (h_e^2 h_f^2) ) ], the
// interior diagonal of L, from the tables of reg_weights (1 for d >= D)
static void solve_centre(const WeightsEL<double> &w, int mode, int D, Diag<double> *c)
{
    double centre = w.abs;
    for (int e = 0; e < D; ++e) {
        centre += w.axis[e][0];
        for (int f = e + 1; f < D; ++f) centre += w.bend2 * w.a1[e][0] * w.a1[f][0];
    }
    for (int d = 0; d < 3; ++d) c->c[d] = d < D ? w.h2[d] * centre : 1.0;
    // (elastic: component d has the centre tap of axo along its own axis; the three-term arithmetic above is untouched)
    if (mode & M_EL)
        for (int d = 0; d < D; ++d) c->c[d] = w.h2[d] * (centre + (w.axo[d][0] - w.axis[d][0]));
}

} // namespace reg
} // namespace ip
