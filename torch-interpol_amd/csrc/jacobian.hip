// ===========================================================================
// jacobian.hip -- Jacobian of the transformation id + u of a voxel displacement field u, at the lattice points.
//
//     J[b, o, d, e] = delta_de + sum_taps (g_e prod_{f != e} w_f)(0) * sign * u[b, wrap(tap), d]
//
// i.e. grid_grad(u as a D-channel image, identity_grid) + identity (reference interpol/pushpull.py:146-172), without the
// channel-first copy of the field, the dense identity grid and the (B, D, *shape, D) intermediate.  The sample points ARE the
// lattice points, so
//   * the first tap is a compile-time offset of the voxel index (no coordinate, no floor) and every weight a constant:
//     the order's B-spline functions of spline_math.hpp at offset 0 (LatticeTaps), folded by the compiler;
//   * taps whose weight AND derivative weight are exactly zero are never loaded: the cubic's fourth tap, and for order 1
//     everything but o and o + e_e (D + 1 loads);
//   * indices and signs are wrap_index / wrap_sign behind the inside test of Stencil::setup (stencil.hpp).
//
//   jac_fwd<R, D, K, DET>    : one thread = one lattice point, in storage order (jac_sample); per tap ONE
//                              D-component load, separable accumulation like grad_generic.  DET = false writes the D x D
//                              matrix, row-major (row = component, column = direction); DET = true expands the determinant
//                              in registers and writes one value -- the matrix field never exists.
//   jacdet_bwd_field<R, D, K>: recomputes J[o] (the same jac_at), multiplies its cofactor matrix by grad_out[o] and stores it in
//                              the layout grid_pushgrad reads, (B, D, *shape, D): the gradient of the determinant with respect
//                              to u is the existing pushgrad of that field along a zero displacement.
//
// No LDS, no workspace, no atomics, no device-side state.  Every thread gathers from `disp`, so no output may overlap it.
// The D-component element has the alignment of ONE component (a view with a storage offset is not 12- or 16-byte aligned).
//
// Instantiated for one order 1..3 in every dim, D = 1..3, float and double.  The C entry points live here as well
// (include/interpol_hip.h: interpol_jacobian, interpol_jacdet_backward_field).
// ===========================================================================
#include "../../include/interpol_hip.h"
#include "ops_generic.hpp"
#include <hip/hip_runtime.h>
#include <string.h>

namespace ip {
namespace jac {

// D components of one lattice point; alignment of a single component (as in compose.hip)
template <typename R, int D> struct PointVec { R c[D]; };
static_assert(alignof(PointVec<float, 3>) == 4 && sizeof(PointVec<float, 3>) == 12, "point-by-point element: 4-byte aligned");
static_assert(alignof(PointVec<double, 3>) == 8 && sizeof(PointVec<double, 3>) == 24, "point-by-point element: 8-byte aligned");

// The stencil of order K at a lattice point x = o.  Stencil::setup has fl = floor(x - (K - 1) / 2) and t = x - fl (nd.py:45-46):
// at an integer x that is fl = o - K / 2 (integer division: o, o - 1, o - 1 for K = 1, 2, 3) and t = K / 2, and tap j has
// the weights of the order's B-spline at t - j -- for K = 1 those of iso1.py:19-20 (w = 1 - t, t; g = -1, +1), which is the
// mode a field with order 1 in every dim runs in (stencil.hpp).  All arguments are constants once the tap loops are
// unrolled, so the functions below fold to literals and `!= 0` tests on them to nothing.
template <typename R, int K> struct LatticeTaps {
    static constexpr int T = K + 1;
    static constexpr int FIRST = -(K / 2);
    static __device__ __forceinline__ R w(int j)
    {
        const R t = R(K / 2);
        return K == 1 ? (j == 0 ? R(1) - t : t) : bspline_w<R>(K, t - R(j));
    }
    static __device__ __forceinline__ R g(int j)
    {
        const R t = R(K / 2);
        return K == 1 ? (j == 0 ? R(-1) : R(1)) : bspline_g<R>(K, t - R(j));
    }
    // does tap j along one dim take part in anything?
    static __device__ __forceinline__ bool live(int j) { return w(j) != R(0) || g(j) != R(0); }
};

// Which lattice point a thread owns: the points in storage order, 256 per workgroup, for every D; od: its D voxel indices.
// -> the linear index of the point, or -1.  In 3-D, boxes of 4 x 2 x 32 (the mapping of compose.hip), 1 x 4 x 64, 1 x 2 x 128 and rows
// of 128 / 256 points per workgroup were timed against this one on 1 x 256^3 x 3, 192 x 200 x 180 and 160 x 160 x 300 float32
// (profiles/jacobian.txt).  No mapping wins everywhere; storage order is first on 256^3, where the 4 x 2 x 32 box is 25 - 35 % behind for
// the order-1 determinant (0.096 against 0.071 - 0.077 ms) and 7 - 14 % for orders 2 - 3, first for the matrix on all three shapes, and
// 5 - 25 % behind the small boxes for the determinant on the two others.  The gathers are lattice aligned whatever the field
// holds, so consecutive points already share their rows and planes in L1 / L2.
template <int D>
__device__ __forceinline__ int64_t jac_sample(const KParams &p, unsigned *od)
{
    od[0] = od[1] = od[2] = 0u;
    const int64_t o = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (o >= p.N) return -1;
    unsigned r = (unsigned)o;                                        // (N < 2^30: one item of the field spans < 4 GiB)
#pragma unroll
    for (int d = D - 1; d > 0; --d) { const unsigned q = r / (unsigned)p.gshape[d]; od[d] = r - q * (unsigned)p.gshape[d]; r = q; }
    od[0] = r;
    return o;
}

// a[c][e] = d/dx_e of component c of the spline of `ub` (one batch item, point by point) at the lattice point od: grad u, no identity
template <typename R, int D, int K>
__device__ __forceinline__ void jac_at(const KParams &p, const PointVec<R, D> *ub, const unsigned *od, R (&a)[D][D])
{
    typedef PointVec<R, D> V;
    typedef LatticeTaps<R, K> W;
    constexpr int T = W::T;
    constexpr int T1 = D > 1 ? T : 1, T2 = D > 2 ? T : 1;
    // weights of tap j along dim d as compile-time values (a dim the field does not have: one tap of weight 1), and the same
    // times the boundary sign as run-time values: (v * s) * w == v * (s * w) exactly for s in {-1, 0, 1} (stencil.hpp)
#define JW(d, j) ((d) < D ? W::w(j) : R(1))
#define JG(d, j) ((d) < D ? W::g(j) : R(0))
    unsigned off[3][T];
    R ws[3][T], gs[3][T];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        if (d >= D) {
#pragma unroll
            for (int j = 0; j < T; ++j) { off[d][j] = 0; ws[d][j] = R(1); gs[d][j] = R(0); }
            continue;
        }
        const int n = p.vol_n[d], bd = p.bound[d], i0 = (int)od[d] + W::FIRST;
        int idx[T], sg[T];
        // the inside test of Stencil::setup over the taps that are loaded (dst1: the sign is 0 at index 0)
        bool inside = i0 >= (bd == B_DST1 ? 1 : 0);
#pragma unroll
        for (int j = 0; j < T; ++j) { idx[j] = i0 + j; sg[j] = 1; if (W::live(j)) inside = inside && (i0 + j < n); }
        if (!inside) {
#pragma unroll
            for (int j = 0; j < T; ++j) {
                if (W::live(j)) {
                    const long long pk = wrap_outofline(bd, i0 + j, n);
                    idx[j] = (int)(pk & 0xffffffffll);
                    sg[j]  = (int)(pk >> 32);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < T; ++j) {
            off[d][j] = W::live(j) ? (unsigned)idx[j] * (unsigned)p.vol_ss[d] : 0u;
            const R sf = R(sg[j]);
            ws[d][j] = W::w(j) * sf;
            gs[d][j] = W::g(j) * sf;
        }
    }
    R a0[D], a1[D], a2[D];
#pragma unroll
    for (int c = 0; c < D; ++c) a0[c] = a1[c] = a2[c] = R(0);
#pragma unroll
    for (int i = 0; i < T; ++i) {
        R pWW[D], pGW[D], pWG[D];
#pragma unroll
        for (int c = 0; c < D; ++c) pWW[c] = pGW[c] = pWG[c] = R(0);
#pragma unroll
        for (int j = 0; j < T1; ++j) {
            const unsigned oij = off[0][i] + off[1][j];
            R rW[D], rG[D];
#pragma unroll
            for (int c = 0; c < D; ++c) rW[c] = rG[c] = R(0);
#pragma unroll
            for (int k = 0; k < T2; ++k) {
                // a tap is loaded when one of the D derivative terms g_e prod_{f != e} w_f is non-zero at it
                const bool t0 = JG(0, i) != R(0) && JW(1, j) != R(0) && JW(2, k) != R(0);
                const bool t1 = JW(0, i) != R(0) && JG(1, j) != R(0) && JW(2, k) != R(0);
                const bool t2 = JW(0, i) != R(0) && JW(1, j) != R(0) && JG(2, k) != R(0);
                if (!(t0 || t1 || t2)) continue;
                const V v = ld_tap(ub, oij + off[2][k]);
#pragma unroll
                for (int c = 0; c < D; ++c) {
                    if (JW(2, k) != R(0)) rW[c] = fma_(ws[2][k], v.c[c], rW[c]);
                    if (D > 2 && JG(2, k) != R(0)) rG[c] = fma_(gs[2][k], v.c[c], rG[c]);
                }
            }
#pragma unroll
            for (int c = 0; c < D; ++c) {
                if (JW(1, j) != R(0)) pWW[c] = fma_(ws[1][j], rW[c], pWW[c]);
                if (D > 1 && JG(1, j) != R(0)) pGW[c] = fma_(gs[1][j], rW[c], pGW[c]);
                if (D > 2 && JW(1, j) != R(0)) pWG[c] = fma_(ws[1][j], rG[c], pWG[c]);
            }
        }
#pragma unroll
        for (int c = 0; c < D; ++c) {
            if (JG(0, i) != R(0)) a0[c] = fma_(gs[0][i], pWW[c], a0[c]);
            if (D > 1 && JW(0, i) != R(0)) a1[c] = fma_(ws[0][i], pGW[c], a1[c]);
            if (D > 2 && JW(0, i) != R(0)) a2[c] = fma_(ws[0][i], pWG[c], a2[c]);
        }
    }
#undef JW
#undef JG
#pragma unroll
    for (int c = 0; c < D; ++c) {
        a[c][0] = a0[c];
        if (D > 1) a[c][1 % D] = a1[c];
        if (D > 2) a[c][2 % D] = a2[c];
    }
}

template <typename R, int D>
__device__ __forceinline__ void add_identity(R (&a)[D][D])
{
#pragma unroll
    for (int c = 0; c < D; ++c) a[c][c] += R(1);
}

// cofactor matrix: cof[d][e] = d det(J) / d J[d][e] (= det(J) J^-T), and the determinant expanded along row 0
template <typename R, int D>
__device__ __forceinline__ R cofactors(const R (&J)[D][D], R (&cof)[D][D])
{
    if (D == 1) { cof[0][0] = R(1); return J[0][0]; }
    if (D == 2) {
        cof[0][0] = J[1 % D][1 % D]; cof[0][1 % D] = -J[1 % D][0];
        cof[1 % D][0] = -J[0][1 % D]; cof[1 % D][1 % D] = J[0][0];
        return J[0][0] * J[1 % D][1 % D] - J[0][1 % D] * J[1 % D][0];
    }
    constexpr int i1 = 1 % D, i2 = 2 % D;
    cof[0][0]   =   J[i1][i1] * J[i2][i2] - J[i1][i2] * J[i2][i1];
    cof[0][i1]  = -(J[i1][0]  * J[i2][i2] - J[i1][i2] * J[i2][0]);
    cof[0][i2]  =   J[i1][0]  * J[i2][i1] - J[i1][i1] * J[i2][0];
    cof[i1][0]  = -(J[0][i1]  * J[i2][i2] - J[0][i2]  * J[i2][i1]);
    cof[i1][i1] =   J[0][0]   * J[i2][i2] - J[0][i2]  * J[i2][0];
    cof[i1][i2] = -(J[0][0]   * J[i2][i1] - J[0][i1]  * J[i2][0]);
    cof[i2][0]  =   J[0][i1]  * J[i1][i2] - J[0][i2]  * J[i1][i1];
    cof[i2][i1] = -(J[0][0]   * J[i1][i2] - J[0][i2]  * J[i1][0]);
    cof[i2][i2] =   J[0][0]   * J[i1][i1] - J[0][i1]  * J[i1][0];
    return J[0][0] * cof[0][0] + J[0][i1] * cof[0][i1] + J[0][i2] * cof[0][i2];
}

// disp (B, *shape, D) through p.vol_sb / p.vol_ss (bytes); out dense per item through p.val_sb: (B, *shape, D, D), or (B, *shape) when DET
template <typename R, int D, int K, bool DET>
__global__ __launch_bounds__(BLOCK) void jac_fwd(KParams p, const R *__restrict__ disp, R *__restrict__ out, int B, int add_id)
{
    typedef PointVec<R, D> V;
    unsigned od[3];
    const int64_t o = jac_sample<D>(p, od);
    if (o < 0) return;
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        R J[D][D];
        jac_at<R, D, K>(p, reinterpret_cast<const V *>(disp + b * p.vol_sb), od, J);
        if (DET) {
            add_identity<R, D>(J);
            R cof[D][D];
            out[b * p.val_sb + o] = cofactors<R, D>(J, cof);
        } else {
            if (add_id) add_identity<R, D>(J);
            V *ob = reinterpret_cast<V *>(out + b * p.val_sb + o * (D * D));
#pragma unroll
            for (int c = 0; c < D; ++c) {
                V row;
#pragma unroll
                for (int e = 0; e < D; ++e) row.c[e] = J[c][e];
                ob[c] = row;
            }
        }
    }
}

// gout (B, *shape) dense; gfield (B, D, *shape, D) dense per item through p.val_sb: gfield[b, d, o, e] = gout[b, o] * cof(J[b, o])[d][e]
template <typename R, int D, int K>
__global__ __launch_bounds__(BLOCK) void jacdet_bwd_field(KParams p, const R *__restrict__ gout, const R *__restrict__ disp,
                                                          R *__restrict__ gfield, int B)
{
    typedef PointVec<R, D> V;
    unsigned od[3];
    const int64_t o = jac_sample<D>(p, od);
    if (o < 0) return;
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        R J[D][D], cof[D][D];
        jac_at<R, D, K>(p, reinterpret_cast<const V *>(disp + b * p.vol_sb), od, J);
        add_identity<R, D>(J);
        cofactors<R, D>(J, cof);
        const R go = gout[b * p.N + o];
        R *gb = gfield + b * p.val_sb + o * D;
#pragma unroll
        for (int c = 0; c < D; ++c) {
            V row;
#pragma unroll
            for (int e = 0; e < D; ++e) row.c[e] = go * cof[c][e];
            *reinterpret_cast<V *>(gb + (int64_t)c * p.N * D) = row;
        }
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------
// Validate + convert (the conventions of compose_params): vol_* is the field, val_stride[0] the batch stride of the output,
// whose items are dense with `per_item` elements per lattice point.
static int jac_params(const interpol_problem *p, int64_t per_item, KParams *k, int *B)
{
    if (!p) return INTERPOL_E_NULL;
    if (p->abi_version != INTERPOL_ABI_VERSION) return INTERPOL_E_SHAPE;
    if (p->dim < 1 || p->dim > 3) return INTERPOL_E_DIM;
    if (p->dtype != INTERPOL_F32 && p->dtype != INTERPOL_F64) return INTERPOL_E_DTYPE;
    if (p->batch < 1 || p->batch > 0x7fffffff || p->channels != p->dim) return INTERPOL_E_SHAPE;
    const int D = p->dim;
    const uint64_t es = p->dtype == INTERPOL_F64 ? 8 : 4;
    memset(k, 0, sizeof(*k));
    k->dim = D;
    k->extrapolate = 1;                                             // lattice points are in bounds
    for (int d = 0; d < D; ++d) {
        if (p->order[d] < 0 || p->order[d] > 7) return INTERPOL_E_ORDER;
        if (p->bound[d] < 0 || p->bound[d] > 6) return INTERPOL_E_BOUND;
        if (p->vol_shape[d] < 1 || p->vol_shape[d] > 0x3fffffff) return INTERPOL_E_SHAPE;
    }
    for (int d = 0; d < D; ++d)
        if (p->order[d] != p->order[0] || p->order[0] < 1 || p->order[0] > 3) return INTERPOL_E_ORDER;   // one order 1..3
    if (D > 1 && p->vol_stride[1] != 1) return INTERPOL_E_STRIDE;   // row-major, point by point
    int64_t exp = D, N = 1;
    uint64_t bytes = (uint64_t)D * es;
    for (int d = D - 1; d >= 0; --d) {
        if (p->vol_shape[d] > 1 && p->vol_stride[2 + d] != exp) return INTERPOL_E_STRIDE;
        k->vol_ss[d] = (int)((uint64_t)exp * es);                   // (< 2^32: one item of the field is, below)
        bytes *= (uint64_t)p->vol_shape[d];
        if (bytes > 0xffffffffull) return INTERPOL_E_SHAPE;         // one item of the field must fit 32-bit byte offsets
        exp *= p->vol_shape[d];
        N *= p->vol_shape[d];
    }
    if (p->vol_stride[0] < 0 || p->val_stride[0] < 0) return INTERPOL_E_STRIDE;
    if (p->batch > 1 && p->val_stride[0] < N * per_item) return INTERPOL_E_STRIDE;   // the output has an item of its own per batch item
    for (int d = 0; d < 3; ++d) {
        if (d >= D) { k->bound[d] = 1; k->order[d] = 0; k->vol_n[d] = 1; k->vol_ss[d] = 0; k->gshape[d] = 1; continue; }
        k->bound[d] = p->bound[d];
        k->order[d] = p->order[d];
        k->vol_n[d] = (int)p->vol_shape[d];
        k->gshape[d] = (int)p->vol_shape[d];
    }
    k->mode = p->order[0] == 1 ? MODE_ISO1 : MODE_ND;
    k->C = D;
    k->N = N;
    k->vol_sb = p->vol_stride[0];
    k->vol_sc = 1;
    k->val_sb = p->val_stride[0];
    k->val_sc = 1;
    *B = (int)p->batch;
    return 0;
}

enum { OP_MATRIX = 0, OP_DET = 1, OP_BWD = 2 };

template <typename R, int D, int K>
static int jac_launch(int op, const KParams &k, const void *gout, const void *disp, void *out, int add_id, int B, hipStream_t st)
{
    const int64_t nb = (k.N + BLOCK - 1) / BLOCK;                   // (< 2^22: N < 2^30)
    const dim3 grid((unsigned)nb, (unsigned)(B < 65535 ? B : 65535), 1);
    if (op == OP_BWD)
        hipLaunchKernelGGL((jacdet_bwd_field<R, D, K>), grid, dim3(BLOCK), 0, st, k, (const R *)gout, (const R *)disp, (R *)out, B);
    else if (op == OP_DET)
        hipLaunchKernelGGL((jac_fwd<R, D, K, true>), grid, dim3(BLOCK), 0, st, k, (const R *)disp, (R *)out, B, 1);
    else
        hipLaunchKernelGGL((jac_fwd<R, D, K, false>), grid, dim3(BLOCK), 0, st, k, (const R *)disp, (R *)out, B, add_id);
    return 0;
}

template <typename R, int D>
static int jac_by_order(int op, const KParams &k, const void *gout, const void *disp, void *out, int add_id, int B, hipStream_t st)
{
    switch (k.order[0]) {
    case 1: return jac_launch<R, D, 1>(op, k, gout, disp, out, add_id, B, st);
    case 2: return jac_launch<R, D, 2>(op, k, gout, disp, out, add_id, B, st);
    default: return jac_launch<R, D, 3>(op, k, gout, disp, out, add_id, B, st);
    }
}

template <typename R>
static int jac_by_dim(int op, const KParams &k, const void *gout, const void *disp, void *out, int add_id, int B, hipStream_t st)
{
    switch (k.dim) {
    case 1: return jac_by_order<R, 1>(op, k, gout, disp, out, add_id, B, st);
    case 2: return jac_by_order<R, 2>(op, k, gout, disp, out, add_id, B, st);
    default: return jac_by_order<R, 3>(op, k, gout, disp, out, add_id, B, st);
    }
}

// 0 or a negative INTERPOL_E_* (a failed launch: INTERPOL_E_LAUNCH)
static int jac_entry(const interpol_problem *p, int op, const void *gout, const void *disp, void *out, int add_id, void *stream)
{
    KParams k; int B;
    const int rc = jac_params(p, op == OP_DET ? 1 : (p ? (int64_t)p->dim * p->dim : 1), &k, &B);
    if (rc) return rc;
    if (!disp || !out || (op == OP_BWD && !gout)) return INTERPOL_E_NULL;
    hipStream_t st = (hipStream_t)stream;
    const int lrc = p->dtype == INTERPOL_F64 ? jac_by_dim<double>(op, k, gout, disp, out, add_id, B, st)
                                             : jac_by_dim<float>(op, k, gout, disp, out, add_id, B, st);
    if (lrc) return lrc;
    return hipGetLastError() == hipSuccess ? 0 : INTERPOL_E_LAUNCH;
}

} // namespace jac
} // namespace ip

extern "C" {

int interpol_jacobian(const interpol_problem *p, const void *disp, void *out, int det_only, int add_identity, void *stream)
{
    return ip::jac::jac_entry(p, det_only ? ip::jac::OP_DET : ip::jac::OP_MATRIX, nullptr, disp, out, add_identity ? 1 : 0, stream);
}

int interpol_jacdet_backward_field(const interpol_problem *p, const void *grad_out, const void *disp, void *gfield, void *stream)
{
    return ip::jac::jac_entry(p, ip::jac::OP_BWD, grad_out, disp, gfield, 1, stream);
}

} // extern "C"
