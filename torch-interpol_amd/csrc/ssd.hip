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
//   dt::slot_finish<R>      : (data_term.hpp) one workgroup per batch item sums the item's slots in a fixed order and writes
//                             0.5 * sum in R.
//
// No atomics; every workgroup writes its slot, so nothing in the workspace is assumed cleared; the summation tree of an item depends
// on its shape alone: two calls give identical bits, an item gives the same bits alone or inside a batch, and the two launches
// replay from a captured graph to the bits of eager.
// `weight` is a nullable pointer (block-uniform branch), not a template parameter.  HK: 0 no Hessian, 1 diagonal, 2 full.
//
// Instantiated for one order 1..3 in every dim, D = 1..3, float and double, HK = 0..2.  The C entry points live here as well
// (include/interpol_hip.h: interpol_ssd_workspace, interpol_ssd).  data_term.hpp holds what the data terms share: the validation of
// the problem (problem_params), the alias check (ranges_alias), HK_* / hess_components / diag_first_index, the stencil loop of one
// channel (IP_STENCIL_VALUE_GRADIENT), the finish and the dispatch on dtype, dim and order.
// ===========================================================================
#include "data_term.hpp"
#include "point_field.hpp"                                         // PointVec, compose_sample, compose_blocks

namespace ip {
namespace ssd {

using namespace dt;

// the batch strides (elements) the problem descriptor has no field for (a kernel parameter: its namespace is part of the kernels' names)
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
                IP_STENCIL_VALUE_GRADIENT(s, v0, aw, a0, a1, a2);
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
                            for (int e = d + 1; e < D; ++e) ha[diag_first_index(d, e, D)] = fma_(g[d], g[e], ha[diag_first_index(d, e, D)]);
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

// ---- host side --------------------------------------------------------------------------------------------------------
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
    hipLaunchKernelGGL((slot_finish<R>), dim3(by), dim3(BLOCK), 0, a.st, (const double *)a.slots, (R *)a.loss, a.nb, a.B, 0.5);
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

} // namespace ssd
} // namespace ip

extern "C" {

int64_t interpol_ssd_workspace(const interpol_problem *p)
{
    ip::KParams k; int B; uint64_t mspan;
    const int rc = ip::dt::problem_params(p, ip::dt::LATTICE_FIELD, &k, &B, &mspan);
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
    Args a;
    uint64_t mimage;
    const int rc = problem_params(p, LATTICE_FIELD, &a.k, &a.B, &mimage);
    if (rc) return rc;
    if (hessian_kind != HK_NONE && hessian_kind != HK_DIAG && hessian_kind != HK_FULL) return INTERPOL_E_SHAPE;
    a.hk = hessian_kind;
    a.nb = ssd_blocks(a.k);
    if (a.nb > 0x7fffffffll) return INTERPOL_E_SHAPE;
    const int D = a.k.dim, K = hess_components(D, a.hk);
    const uint64_t B = (uint64_t)a.B, N = (uint64_t)a.k.N;
    const uint64_t es = p->dtype == INTERPOL_F64 ? 8 : 4;
    if (gradient_batch_stride < 0 || (weight && weight_batch_stride < 0) || (K && hessian_batch_stride < 0)) return INTERPOL_E_STRIDE;
    // the outputs have an item of their own per batch item
    if (B > 1 && ((uint64_t)gradient_batch_stride < N * D || (K && (uint64_t)hessian_batch_stride < N * K))) return INTERPOL_E_STRIDE;
    if (!moving || !fixed || !disp || !loss || !gradient || !workspace || (K && !hessian)) return INTERPOL_E_NULL;
    if ((uintptr_t)workspace % sizeof(double)) return INTERPOL_E_STRIDE;             // (the slots are doubles)
    const uint64_t wsbytes = B * (uint64_t)a.nb * sizeof(double);
    if (workspace_bytes < (int64_t)wsbytes) return INTERPOL_E_SCRATCH;
    // what is written (loss, gradient, hessian, workspace) overlaps neither an input nor each other
    const Range rd[4] = { { moving, moving_bytes(a.k, B, es, mimage) }, { fixed, fixed_bytes(a.k, B, es) },
                          { disp, ((B - 1) * (uint64_t)a.k.grid_sb + N * D) * es }, { weight, weight_bytes(a.k, B, es, weight, weight_batch_stride) } };
    const Range wr[4] = { { loss, B * es }, { gradient, ((B - 1) * (uint64_t)gradient_batch_stride + N * D) * es },
                          { hessian, K ? ((B - 1) * (uint64_t)hessian_batch_stride + N * K) * es : 0 }, { workspace, wsbytes } };
    if (ranges_alias(rd, 4, wr, 4)) return INTERPOL_E_STRIDE;
    a.sb.weight = weight ? weight_batch_stride : 0;
    a.sb.gradient = gradient_batch_stride;
    a.sb.hessian = K ? hessian_batch_stride : 0;                    // (no Hessian: never dereferenced)
    a.moving = moving; a.fixed = fixed; a.disp = disp; a.weight = weight;
    a.loss = loss; a.gradient = gradient; a.hessian = K ? hessian : nullptr;
    a.slots = (double *)workspace; a.st = (hipStream_t)stream;
    dispatch(p, a.k, [&](auto r, auto d, auto kmax) { ssd_by_hessian<decltype(r), decltype(d)::value, decltype(kmax)::value>(a); });
    return hipGetLastError() == hipSuccess ? 0 : INTERPOL_E_LAUNCH;
}

} // extern "C"
