// ===========================================================================
// compose.hip -- composition of two voxel displacement fields, point by point.
//
//     out[b, o, :] = right[b, o, :] + mask(x) * sum_taps W(x) * sign * left[b, wrap(tap), :],     x = o + right[b, o, :]
//
// i.e. right + grid_pull(left as a D-channel image, right, displacement = True) (reference interpol/pushpull.py:35-66
// behind add_identity_grid, api.py:490-531) without the channel-first detour: a displacement field is stored
// (B, *shape, D), so ONE address computation per tap fetches all D components of `left` in one 4 D-byte (8 D for
// double) load, and the result is written where `right` was read, in the same layout.  Scaling and squaring
// (u <- u o (id + u)) is this kernel `steps` times.
//
//   compose_fwd       : one thread = one sample (3-D: a workgroup owns a box of samples, see compose_sample);
//                       coordinates by the displacement branch of load_coords, indices / signs /
//                       weights / mask by Stencil<R, D, K, ISO, NEED_W> (stencil.hpp: the one statement of those rules);
//                       per tap one D-component load and D FMAs; separable accumulation like pull_generic.
//   compose_bwd_right : the same with NEED_G.  gright[e] = gout[e] + mask * sum_d gout[d] * dL_d/dx_e: the D x D contraction
//                       with gout is taken per tap (s = <gout, left[tap]>, one D-component load and D FMAs), the D
//                       derivative sums then run on the scalar s as in grad_generic.
//
// No LDS, no workspace, no atomics, no device-side state: every thread reads its own element of `right` (`grad_out`) before
// it writes the same element of `out` (`grad_right`), so `out` may alias `right`; it must not alias `left`.
// The D-component element is declared with the alignment of ONE component: a view with a storage offset is not 12- or
// 16-byte aligned.
//
// Instantiated for one order 1..3 in every dim, D = 1..3, float and double.  The C entry points live here as well
// (include/interpol_hip.h: interpol_compose, interpol_compose_backward_right).
// ===========================================================================
#include "../../include/interpol_hip.h"
#include "point_field.hpp"                                         // PointVec, compose_sample, compose_blocks
#include <hip/hip_runtime.h>
#include <string.h>

namespace ip {

// left (B, *lshape, D) through p.vol_sb / p.vol_ss (bytes), right and out (B, *oshape, D) through p.grid_sb / p.val_sb
template <typename R, int D, int KMAX>
__global__ __launch_bounds__(BLOCK) void compose_fwd(KParams p, const R *__restrict__ left, const R *right, R *out, int B)
{
    typedef PointVec<R, D> V;
    const int64_t o = compose_sample<D>(p);
    if (o < 0) return;
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        R x[D];
        load_coords<R, R, D>(p, right, b, o, x);
        const V r = *reinterpret_cast<const V *>(right + b * p.grid_sb + o * D);
        Stencil<R, D, KMAX, true, NEED_W> s;
        s.setup(p, x);
        const V *lb = reinterpret_cast<const V *>(left + b * p.vol_sb);
        R a[D];
#pragma unroll
        for (int e = 0; e < D; ++e) a[e] = R(0);
        IP_FOR_I {
            R pj[D];
#pragma unroll
            for (int e = 0; e < D; ++e) pj[e] = R(0);
            IP_FOR_J {
                const unsigned oij = s.off[0][i] + s.off[1][j];
                R rk[D];
#pragma unroll
                for (int e = 0; e < D; ++e) rk[e] = R(0);
                IP_FOR_K {
                    const V v = ld_tap(lb, oij + s.off[2][k]);
#pragma unroll
                    for (int e = 0; e < D; ++e) rk[e] = fma_(s.w[2][k], v.c[e], rk[e]);
                } IP_ROW_END;
#pragma unroll
                for (int e = 0; e < D; ++e) pj[e] = fma_(s.w[1][j], rk[e], pj[e]);
            }
#pragma unroll
            for (int e = 0; e < D; ++e) a[e] = fma_(s.w[0][i], pj[e], a[e]);
        }
        V res;
#pragma unroll
        for (int e = 0; e < D; ++e) res.c[e] = r.c[e] + a[e] * s.mask;
        *reinterpret_cast<V *>(out + b * p.val_sb + o * D) = res;
    }
}

// gout and gright (B, *oshape, D) through p.val_sb
template <typename R, int D, int KMAX>
__global__ __launch_bounds__(BLOCK) void compose_bwd_right(KParams p, const R *gout, const R *__restrict__ left,
                                                           const R *__restrict__ right, R *gright, int B)
{
    typedef PointVec<R, D> V;
    const int64_t o = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (o >= p.N) return;
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        R x[D];
        load_coords<R, R, D>(p, right, b, o, x);
        const V go = *reinterpret_cast<const V *>(gout + b * p.val_sb + o * D);
        Stencil<R, D, KMAX, true, NEED_G> s;
        s.setup(p, x);
        const V *lb = reinterpret_cast<const V *>(left + b * p.vol_sb);
        R a0 = R(0), a1 = R(0), a2 = R(0);
        IP_FOR_I {
            R pWW = R(0), pGW = R(0), pWG = R(0);
            IP_FOR_J {
                const unsigned oij = s.off[0][i] + s.off[1][j];
                R rW = R(0), rG = R(0);
                IP_FOR_K {
                    const V l = ld_tap(lb, oij + s.off[2][k]);
                    R v = go.c[0] * l.c[0];
#pragma unroll
                    for (int d = 1; d < D; ++d) v = fma_(go.c[d], l.c[d], v);
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
        const R acc[3] = { a0, a1, a2 };
        V res;
#pragma unroll
        for (int e = 0; e < D; ++e) res.c[e] = go.c[e] + acc[e] * s.mask;
        *reinterpret_cast<V *>(gright + b * p.val_sb + o * D) = res;
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------
// Validate + convert: vol_* is left's lattice, grid_* is right, val_* is out / grad_out / grad_right.  All three point by
// point, row-major, component stride 1.
static int compose_params(const interpol_problem *p, KParams *k, int *B)
{
    if (!p) return INTERPOL_E_NULL;
    if (p->abi_version != INTERPOL_ABI_VERSION) return INTERPOL_E_SHAPE;
    if (p->dim < 1 || p->dim > 3) return INTERPOL_E_DIM;
    if (p->extrapolate < 0 || p->extrapolate > 2) return INTERPOL_E_EXTRAP;
    if (p->dtype != INTERPOL_F32 && p->dtype != INTERPOL_F64) return INTERPOL_E_DTYPE;
    if (p->grid_dtype != p->dtype) return INTERPOL_E_DTYPE;
    if (p->batch < 1 || p->batch > 0x7fffffff || p->channels != p->dim) return INTERPOL_E_SHAPE;
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
    // row-major point-by-point layouts
    if (D > 1 && (p->vol_stride[1] != 1 || p->grid_stride[4] != 1 || p->val_stride[1] != 1)) return INTERPOL_E_STRIDE;
    int64_t lexp = D, oexp = D, N = 1;
    uint64_t lbytes = (uint64_t)D * es;
    for (int d = D - 1; d >= 0; --d) {
        if (p->vol_shape[d] > 1 && p->vol_stride[2 + d] != lexp) return INTERPOL_E_STRIDE;
        if (p->grid_shape[d] > 1 && (p->grid_stride[1 + d] != oexp || p->val_stride[2 + d] != oexp)) return INTERPOL_E_STRIDE;
        k->vol_ss[d] = (int)((uint64_t)lexp * es);                  // (< 2^32: one item of left is, below)
        lbytes *= (uint64_t)p->vol_shape[d];
        if (lbytes > 0xffffffffull) return INTERPOL_E_SHAPE;        // one item of left must fit 32-bit byte offsets
        lexp *= p->vol_shape[d];
        oexp *= p->grid_shape[d];
        N *= p->grid_shape[d];
        if (N > 0xffffffffll) return INTERPOL_E_SHAPE;              // the sample index is split in 32 bits (load_coords)
    }
    if (p->vol_stride[0] < 0 || p->grid_stride[0] < 0 || p->val_stride[0] < 0) return INTERPOL_E_STRIDE;
    if (p->batch > 1 && p->val_stride[0] < oexp) return INTERPOL_E_STRIDE;      // the output has an item of its own per batch item
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
    k->C = D;
    k->sep = 2;                                                     // `right` holds displacements: load_coords adds the lattice
    k->N = N;
    k->vol_sb = p->vol_stride[0];
    k->vol_sc = 1;
    k->grid_sb = p->grid_stride[0];
    k->val_sb = p->val_stride[0];
    k->val_sc = 1;
    *B = (int)p->batch;
    return 0;
}

template <typename R, int D, int K>
static int compose_launch(bool bwd, const KParams &k, const void *a, const void *left, const void *right, void *out, int B, hipStream_t st)
{
    const int64_t nb = bwd ? (k.N + BLOCK - 1) / BLOCK : compose_blocks<D>(k);
    if (nb > 0x7fffffffll) return INTERPOL_E_SHAPE;                 // (a thin 3-D lattice of more than 2^31 boxes)
    const dim3 grid((unsigned)nb, (unsigned)(B < 65535 ? B : 65535), 1);
    if (bwd)
        hipLaunchKernelGGL((compose_bwd_right<R, D, K>), grid, dim3(BLOCK), 0, st, k, (const R *)a, (const R *)left, (const R *)right, (R *)out, B);
    else
        hipLaunchKernelGGL((compose_fwd<R, D, K>), grid, dim3(BLOCK), 0, st, k, (const R *)left, (const R *)right, (R *)out, B);
    return 0;
}

template <typename R, int D>
static int compose_by_order(bool bwd, const KParams &k, const void *a, const void *left, const void *right, void *out, int B, hipStream_t st)
{
    switch (k.order[0]) {
    case 1: return compose_launch<R, D, 1>(bwd, k, a, left, right, out, B, st);
    case 2: return compose_launch<R, D, 2>(bwd, k, a, left, right, out, B, st);
    default: return compose_launch<R, D, 3>(bwd, k, a, left, right, out, B, st);
    }
}

template <typename R>
static int compose_by_dim(bool bwd, const KParams &k, const void *a, const void *left, const void *right, void *out, int B, hipStream_t st)
{
    switch (k.dim) {
    case 1: return compose_by_order<R, 1>(bwd, k, a, left, right, out, B, st);
    case 2: return compose_by_order<R, 2>(bwd, k, a, left, right, out, B, st);
    default: return compose_by_order<R, 3>(bwd, k, a, left, right, out, B, st);
    }
}

// a: grad_out of the backward, NULL for the forward.  0 or a negative INTERPOL_E_* (a failed launch: INTERPOL_E_LAUNCH).
static int compose_entry(const interpol_problem *p, bool bwd, const void *a, const void *left, const void *right, void *out, void *stream)
{
    KParams k; int B;
    const int rc = compose_params(p, &k, &B);
    if (rc) return rc;
    if (!left || !right || !out || (bwd && !a)) return INTERPOL_E_NULL;
    hipStream_t st = (hipStream_t)stream;
    const int lrc = p->dtype == INTERPOL_F64 ? compose_by_dim<double>(bwd, k, a, left, right, out, B, st)
                                             : compose_by_dim<float>(bwd, k, a, left, right, out, B, st);
    if (lrc) return lrc;
    return hipGetLastError() == hipSuccess ? 0 : INTERPOL_E_LAUNCH;
}

} // namespace ip

extern "C" {

int interpol_compose(const interpol_problem *p, const void *left, const void *right, void *out, void *stream)
{
    return ip::compose_entry(p, false, nullptr, left, right, out, stream);
}

int interpol_compose_backward_right(const interpol_problem *p, const void *grad_out, const void *left, const void *right,
                                    void *grad_right, void *stream)
{
    return ip::compose_entry(p, true, grad_out, left, right, grad_right, stream);
}

} // extern "C"
