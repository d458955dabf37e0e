// ===========================================================================
// ssd.hip -- the sum-of-squares data term of a Gauss-Newton registration step: loss, gradient and Hessian in one pass.
//
//     w_c(o)  = mask(x) sum_taps W(x) sign moving[b, c, wrap(tap)],        x = o + disp[b, o, :]          (= grid_pull)
//     G_cd(o) = mask(x) sum_taps dW/dx_d(x) sign moving[b, c, wrap(tap)]                                   (= grid_grad)
//     r_c     = w_c - fixed[b, c, o]
//     loss[b]           = 1/2 sum_o sum_c weight[b, o] r_c^2
//     gradient[b, o, d] = weight[b, o] sum_c r_c G_cd
//     hessian[b, o, k]  = weight[b, o] sum_c G_cd G_ce       k: the diagonal first, then the upper triangle row by row
//
// -- the `gradient` and `hessian` that regulariser_solve.hip takes.  The composed form (grid_pull, grid_grad and a dozen
// element-wise passes) sets the stencil up twice and sends w and G through memory; here neither is ever stored.
//
//   ssd_fwd<R, D, KMAX, HK> : one thread = one sample (3-D: a workgroup owns a box of samples, point_field.hpp: compose_sample);
//                             coordinates by the displacement branch of load_coords; ONE Stencil<R, D, K, ISO, NEED_G> per sample,
//                             (NEED_* is a level: NEED_G holds the value weights as well as the derivative weights)
//                             reused by every channel; per channel the value and the D derivative sums are accumulated
//                             separably (grad_generic plus one FMA per first-dim tap for the value), then r_c and the D + K
//                             products go into register accumulators.  One PointVec<R, D> and one PointVec<R, K> store per sample.
//                             weight r_c^2 is formed in R and summed in DOUBLE: over the channels in the thread, then
//                             block_sum1, one double per workgroup into its own slot of the workspace.
//   ssd_finish<R>           : one workgroup per batch item sums the item's slots in a fixed order (FINISH_WAYS partial sums per
//                             thread, then block_sum1) and writes 0.5 * sum in R.
//
// No atomics; every workgroup writes its slot, so nothing in the workspace is assumed cleared; the summation tree of an item depends
// on its shape alone: two calls give identical bits, an item gives the same bits alone or inside a batch, and the two launches
// replay from a captured graph to the bits of eager.
// `weight` is a nullable pointer (block-uniform branch), not a template parameter.  HK: 0 no Hessian, 1 diagonal, 2 full.
//
// Instantiated for one order 1..3 in every dim, D = 1..3, float and double, HK = 0..2.  The C entry points live here as well
// (include/interpol_hip.h: interpol_ssd_workspace, interpol_ssd).
// ===========================================================================
#include "../../include/interpol_hip.h"
#include "point_field.hpp"                                         // PointVec, compose_sample, compose_blocks
#include "regulariser_at.hpp"                                      // block_sum1, ranges_overlap
#include <hip/hip_runtime.h>
#include <string.h>

namespace ip {
namespace ssd {

enum { HK_NONE = 0, HK_DIAG = 1, HK_FULL = 2 };

constexpr int hess_components(int D, int hk) { return hk == HK_NONE ? 0 : (hk == HK_DIAG ? D : D * (D + 1) / 2); }

// the batch strides (elements) the problem descriptor has no field for
struct Strides { int64_t weight, gradient, hessian; };

// moving (B, C, *in) through p.vol_sb / p.vol_sc / p.vol_ss (bytes), disp (B, *shape, D) through p.grid_sb, fixed (B, C, *shape)
// through p.val_sb / p.val_sc; slots (B, gridDim.x) doubles
template <typename R, int D, int KMAX, int HK>
__global__ __launch_bounds__(BLOCK) void ssd_fwd(KParams p, const R *__restrict__ moving, const R *__restrict__ fixed,
                                                 const R *__restrict__ disp, const R *__restrict__ weight, R *__restrict__ gradient,
                                                 R *__restrict__ hessian, double *__restrict__ slots, Strides sb, int B)
{
    constexpr int K = HK == HK_NONE ? 1 : hess_components(D, HK);
    typedef PointVec<R, D> V;
    typedef PointVec<R, K> H;
    __shared__ double part[BLOCK / 64];
    const int64_t o = compose_sample<D>(p);                         // < 0: a thread past the lattice (it still takes part in the sum)
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        double loss = 0.0;
        if (o >= 0) {
            R x[D];
            load_coords<R, R, D>(p, disp, b, o, x);
            Stencil<R, D, KMAX, true, NEED_G> s;
            s.setup(p, x);
            const R wt = weight ? weight[b * sb.weight + o] : R(1);
            const R *mb = moving + b * p.vol_sb;
            const R *fb = fixed + b * p.val_sb + o;
            R ga[D], ha[K];
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
                const R acc[3] = { a0, a1, a2 };
                R g[D];
#pragma unroll
                for (int d = 0; d < D; ++d) g[d] = acc[d] * s.mask;
                const R r = aw * s.mask - fb[c * p.val_sc];
#pragma unroll
                for (int d = 0; d < D; ++d) ga[d] = fma_(r, g[d], ga[d]);
                if (HK != HK_NONE) {
#pragma unroll
                    for (int d = 0; d < D; ++d) ha[d] = fma_(g[d], g[d], ha[d]);
                    if (HK == HK_FULL) {
#pragma unroll
                        for (int d = 0; d < D; ++d) {
#pragma unroll
                            for (int e = d + 1; e < D; ++e) {
                                const int k = D + d * D - d * (d + 1) / 2 + (e - d - 1);   // the upper triangle row by row
                                ha[k] = fma_(g[d], g[e], ha[k]);
                            }
                        }
                    }
                }
                loss += (double)(wt * (r * r));
            }
            V gv;
#pragma unroll
            for (int d = 0; d < D; ++d) gv.c[d] = wt * ga[d];
            *reinterpret_cast<V *>(gradient + b * sb.gradient + o * D) = gv;
            if (HK != HK_NONE) {
                H hv;
#pragma unroll
                for (int k = 0; k < K; ++k) hv.c[k] = wt * ha[k];
                *reinterpret_cast<H *>(hessian + b * sb.hessian + o * K) = hv;
            }
        }
        const double t = reg::block_sum1(loss, part);
        if (threadIdx.x == 0) slots[b * gridDim.x + blockIdx.x] = t;
    }
}

constexpr int FINISH_WAYS = 8;

// slots (B, nslots) doubles -> loss (B)
template <typename R>
__global__ __launch_bounds__(BLOCK) void ssd_finish(const double *__restrict__ slots, R *__restrict__ loss, int64_t nslots, int B)
{
    __shared__ double part[BLOCK / 64];
    for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
        // FINISH_WAYS independent partial sums per thread, so that the loads of a round are in flight together (one sum per thread
        // is a chain of nslots / BLOCK dependent loads: 90 us at 256^3); which slot goes into which sum depends on nslots alone
        const double *sl = slots + b * nslots;
        double a[FINISH_WAYS];
#pragma unroll
        for (int j = 0; j < FINISH_WAYS; ++j) a[j] = 0.0;
        int64_t r = threadIdx.x;
        for (; r + (FINISH_WAYS - 1) * BLOCK < nslots; r += FINISH_WAYS * BLOCK) {
#pragma unroll
            for (int j = 0; j < FINISH_WAYS; ++j) a[j] += sl[r + j * BLOCK];
        }
#pragma unroll
        for (int j = 0; j < FINISH_WAYS - 1; ++j)                   // the last, partial round
            if (r + j * BLOCK < nslots) a[j] += sl[r + j * BLOCK];
#pragma unroll
        for (int w = FINISH_WAYS / 2; w > 0; w /= 2) {
#pragma unroll
            for (int j = 0; j < w; ++j) a[j] += a[j + w];
        }
        const double t = reg::block_sum1(a[0], part);
        if (threadIdx.x == 0) loss[b] = (R)(0.5 * t);
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------
// Validate + convert: vol_* is moving as interpol_pull takes its vol, grid_* is disp, val_* is fixed as interpol_pull takes its val.
// *mspan: the bytes one (batch, channel) image of moving spans.
static int ssd_params(const interpol_problem *p, KParams *k, int *B, uint64_t *mspan)
{
    if (!p) return INTERPOL_E_NULL;
    if (p->abi_version != INTERPOL_ABI_VERSION) return INTERPOL_E_SHAPE;
    if (p->dim < 1 || p->dim > 3) return INTERPOL_E_DIM;
    if (p->extrapolate < 0 || p->extrapolate > 2) return INTERPOL_E_EXTRAP;
    if (p->dtype != INTERPOL_F32 && p->dtype != INTERPOL_F64) return INTERPOL_E_DTYPE;
    if (p->grid_dtype != p->dtype) return INTERPOL_E_DTYPE;
    if (p->batch < 1 || p->batch > 0x7fffffff || p->channels < 1 || p->channels > 0x7fffffff) return INTERPOL_E_SHAPE;
    if (p->flags & (INTERPOL_FLAG_SEPARABLE_GRID | INTERPOL_FLAG_AFFINE_GRID)) return INTERPOL_E_STRIDE;   // disp is a dense field
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
    // disp and fixed: row-major over the sample lattice
    if (D > 1 && p->grid_stride[4] != 1) return INTERPOL_E_STRIDE;
    int64_t gexp = D, fexp = 1, N = 1;
    for (int d = D - 1; d >= 0; --d) {
        if (p->grid_shape[d] > 1 && (p->grid_stride[1 + d] != gexp || p->val_stride[2 + d] != fexp)) return INTERPOL_E_STRIDE;
        gexp *= p->grid_shape[d];
        fexp *= p->grid_shape[d];
        N *= p->grid_shape[d];
        if (N > 0xffffffffll) return INTERPOL_E_SHAPE;              // the sample index is split in 32 bits (load_coords)
    }
    if (p->vol_stride[0] < 0 || p->vol_stride[1] < 0 || p->grid_stride[0] < 0 || p->val_stride[0] < 0 || p->val_stride[1] < 0)
        return INTERPOL_E_STRIDE;
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
    k->sep = 2;                                                     // `disp` holds displacements: load_coords adds the lattice
    k->N = N;
    k->vol_sb = p->vol_stride[0];
    k->vol_sc = p->vol_stride[1];
    k->grid_sb = p->grid_stride[0];
    k->val_sb = p->val_stride[0];
    k->val_sc = p->val_stride[1];
    *B = (int)p->batch;
    return 0;
}

// workgroups of ssd_fwd per batch item = doubles per item in the workspace: a function of the sample lattice alone
static int64_t ssd_blocks(const KParams &k)
{
    switch (k.dim) {
    case 1: return compose_blocks<1>(k);
    case 2: return compose_blocks<2>(k);
    default: return compose_blocks<3>(k);
    }
}

struct Args {
    KParams k; int B; int hk; int64_t nb; Strides sb;
    const void *moving, *fixed, *disp, *weight; void *loss, *gradient, *hessian; double *slots; hipStream_t st;
};

template <typename R, int D, int KMAX, int HK>
static void ssd_launch(const Args &a)
{
    const unsigned by = (unsigned)(a.B < 65535 ? a.B : 65535);
    hipLaunchKernelGGL((ssd_fwd<R, D, KMAX, HK>), dim3((unsigned)a.nb, by, 1), dim3(BLOCK), 0, a.st, a.k, (const R *)a.moving,
                       (const R *)a.fixed, (const R *)a.disp, (const R *)a.weight, (R *)a.gradient, (R *)a.hessian, a.slots, a.sb, a.B);
    hipLaunchKernelGGL((ssd_finish<R>), dim3(by), dim3(BLOCK), 0, a.st, (const double *)a.slots, (R *)a.loss, a.nb, a.B);
}

template <typename R, int D, int KMAX>
static void ssd_by_hessian(const Args &a)
{
    switch (a.hk) {
    case HK_NONE: return ssd_launch<R, D, KMAX, HK_NONE>(a);
    case HK_DIAG: return ssd_launch<R, D, KMAX, HK_DIAG>(a);
    default: return ssd_launch<R, D, KMAX, HK_FULL>(a);
    }
}

template <typename R, int D>
static void ssd_by_order(const Args &a)
{
    switch (a.k.order[0]) {
    case 1: return ssd_by_hessian<R, D, 1>(a);
    case 2: return ssd_by_hessian<R, D, 2>(a);
    default: return ssd_by_hessian<R, D, 3>(a);
    }
}

template <typename R>
static void ssd_by_dim(const Args &a)
{
    switch (a.k.dim) {
    case 1: return ssd_by_order<R, 1>(a);
    case 2: return ssd_by_order<R, 2>(a);
    default: return ssd_by_order<R, 3>(a);
    }
}

} // namespace ssd
} // namespace ip

extern "C" {

int64_t interpol_ssd_workspace(const interpol_problem *p)
{
    ip::KParams k; int B; uint64_t mspan;
    const int rc = ip::ssd::ssd_params(p, &k, &B, &mspan);
    if (rc) return rc;
    const int64_t nb = ip::ssd::ssd_blocks(k);
    if (nb > 0x7fffffffll) return INTERPOL_E_SHAPE;                 // (a thin 3-D lattice of more than 2^31 boxes)
    return (int64_t)B * nb * (int64_t)sizeof(double);
}

int interpol_ssd(const interpol_problem *p, const void *moving, const void *fixed, const void *disp, const void *weight,
                 void *loss, void *gradient, void *hessian, int hessian_kind, int64_t weight_batch_stride,
                 int64_t gradient_batch_stride, int64_t hessian_batch_stride, void *workspace, int64_t workspace_bytes, void *stream)
{
    using namespace ip::ssd;
    using ip::reg::ranges_overlap;
    Args a;
    uint64_t mimage;
    const int rc = ssd_params(p, &a.k, &a.B, &mimage);
    if (rc) return rc;
    if (hessian_kind != HK_NONE && hessian_kind != HK_DIAG && hessian_kind != HK_FULL) return INTERPOL_E_SHAPE;
    a.hk = hessian_kind;
    a.nb = ssd_blocks(a.k);
    if (a.nb > 0x7fffffffll) return INTERPOL_E_SHAPE;
    const int D = a.k.dim, K = hess_components(D, a.hk);
    const uint64_t B = (uint64_t)a.B, N = (uint64_t)a.k.N, C = (uint64_t)a.k.C;
    const uint64_t es = p->dtype == INTERPOL_F64 ? 8 : 4;
    if (gradient_batch_stride < 0 || (weight && weight_batch_stride < 0) || (K && hessian_batch_stride < 0)) return INTERPOL_E_STRIDE;
    // the outputs have an item of their own per batch item
    if (B > 1 && ((uint64_t)gradient_batch_stride < N * D || (K && (uint64_t)hessian_batch_stride < N * K))) return INTERPOL_E_STRIDE;
    if (!moving || !fixed || !disp || !loss || !gradient || !workspace || (K && !hessian)) return INTERPOL_E_NULL;
    if ((uintptr_t)workspace % sizeof(double)) return INTERPOL_E_STRIDE;             // (the slots are doubles)
    const uint64_t wsbytes = B * (uint64_t)a.nb * sizeof(double);
    if (workspace_bytes < (int64_t)wsbytes) return INTERPOL_E_SCRATCH;
    // what is written (loss, gradient, hessian, workspace) overlaps neither an input nor each other
    const void *rd[4] = { moving, fixed, disp, weight };
    const uint64_t rn[4] = { ((B - 1) * (uint64_t)a.k.vol_sb + (C - 1) * (uint64_t)a.k.vol_sc) * es + mimage,
                             ((B - 1) * (uint64_t)a.k.val_sb + (C - 1) * (uint64_t)a.k.val_sc + N) * es,
                             ((B - 1) * (uint64_t)a.k.grid_sb + N * D) * es,
                             weight ? ((B - 1) * (uint64_t)weight_batch_stride + N) * es : 0 };
    const void *wr[4] = { loss, gradient, hessian, workspace };
    const uint64_t wn[4] = { B * es, ((B - 1) * (uint64_t)gradient_batch_stride + N * D) * es,
                             K ? ((B - 1) * (uint64_t)hessian_batch_stride + N * K) * es : 0, wsbytes };
    for (int i = 0; i < 4; ++i) {
        if (!wn[i]) continue;
        for (int j = 0; j < 4; ++j)
            if (rn[j] && ranges_overlap(wr[i], wn[i], rd[j], rn[j])) return INTERPOL_E_STRIDE;
        for (int j = i + 1; j < 4; ++j)
            if (wn[j] && ranges_overlap(wr[i], wn[i], wr[j], wn[j])) return INTERPOL_E_STRIDE;
    }
    a.sb.weight = weight ? weight_batch_stride : 0;
    a.sb.gradient = gradient_batch_stride;
    a.sb.hessian = K ? hessian_batch_stride : 0;                    // (no Hessian: never dereferenced)
    a.moving = moving; a.fixed = fixed; a.disp = disp; a.weight = weight;
    a.loss = loss; a.gradient = gradient; a.hessian = K ? hessian : nullptr;
    a.slots = (double *)workspace; a.st = (hipStream_t)stream;
    if (p->dtype == INTERPOL_F64) ssd_by_dim<double>(a);
    else ssd_by_dim<float>(a);
    return hipGetLastError() == hipSuccess ? 0 : INTERPOL_E_LAUNCH;
}

} // extern "C"
