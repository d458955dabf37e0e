// ===========================================================================
// lcc.hip -- the local (windowed) normalised cross-correlation data term of a Gauss-Newton registration step: loss, gradient and
// the positive part of the Hessian with respect to the displacement field.
//
//     I_c(o)  = mask(x) sum_taps W(x) sign moving[b, c, wrap(tap)],        x = o + disp[b, o, :]          (= grid_pull)
//     G_cd(o) = mask(x) sum_taps dW/dx_d(x) sign moving[b, c, wrap(tap)]                                   (= grid_grad)
//     J_c     = fixed[b, c, o]
//     S_X(o)  = sum of X over the window |p_d - o_d| <= r_d clipped to the lattice, n(o) its number of points;  X in I, J, I^2, J^2, IJ
//     cross = S_IJ - S_I S_J / n,  vI = max(S_II - S_I^2 / n, 0),  vJ = max(S_JJ - S_J^2 / n, 0),  den = vI vJ + eps,  cc = cross^2 / den
//     a = weight 2 cross / den,   c = weight 2 cross^2 vJ / den^2,   f = (a S_J - c S_I) / n;    A, C, F = their window sums
//     dI = -J A + I C + F
//     loss[b]           = - sum_o weight(o) sum_c cc_c(o)
//     gradient[b, o, d] = sum_c dI_c G_cd
//     hessian[b, o, k]  = sum_c C_c G_cd G_ce                    k: the diagonal first, then the upper triangle row by row
//
// Three stages, all on the caller's stream:
//   lcc_pull<R, D, KMAX>      : one thread = one sample (point_field.hpp: compose_sample), the Stencil of ssd_fwd at the level of the
//                               values, evaluated in DOUBLE at the coordinate formed in R; writes I (B, C, N), rounded to R once.
//   lcc_stats<R, WX>          : the window sums of I, J, I^2, J^2, IJ (the products and every sum in DOUBLE; R = double with a ring of
//                               up to five planes: in PAIRS of doubles that carry the rounding errors, see Stats) and the per-voxel
//                               epilogue down to a, c, f (doubles: B, C, 3, N in the workspace); weight cc is summed in
//                               double per thread, then block_sum1, one double per workgroup into its own slot.  dt::slot_finish
//                               (data_term.hpp) sums the slots and writes minus the sum.
//   lcc_back<R, D, KMAX, WX>  : the window sums of a, c, f (double); the epilogue forms dI (double, rounded to R once), evaluates the
//                               stencil of `moving` again for G and stores gradient and Hessian with scalar stores.
//
// The window sum (window_march) is the hot path.  The lattice is taken as 3-D (x, y, z; z fastest; leading extents of 1 and radii
// of 0 for D < 3).  A workgroup owns a TILE of TY x TZ = 8 x 32 columns (one per thread) and a chunk of XC = 32 planes along x.  It marches
// along x: per input plane (the chunk plus r_x planes on either side, clipped to the lattice) it
//   1. loads the tile with its halo of (r_y, r_z) into LDS, zeros outside the lattice (the window is clipped, not wrapped),
//   2. sums along z (every row of the halo'd tile), 3. sums along y -- each thread its own column -- into its slot of a RING of WX
//   x-planes in LDS, and 4. once a plane's window is complete, sums the ring's planes in ascending x and runs the epilogue.
// A 9^3 halo tile of five doubles does not fit the LDS; the ring of 9 planes x 5 sums x 256 doubles (90 KiB) does.  Every sum runs
// in a fixed order that depends on the shape and the window alone: no atomics, nothing in the workspace is assumed cleared, two
// calls give identical bits, an item gives the same bits alone or inside a batch, and the launches replay from a captured graph.
//
// Instantiated for one order 1..3 in every dim, D = 1..3, float and double, rings of 1 (D < 3), 5 and 9 planes.  The Hessian kind
// and the weight are run-time (block-uniform) branches.  The C entry points live here as well (include/interpol_hip.h:
// interpol_lcc_workspace, interpol_lcc).  data_term.hpp holds what the data terms share: the validation of the problem
// (problem_params), the alias check (ranges_alias), HK_* / hess_components / diag_first_index, the stencil loops of one channel
// (IP_STENCIL_VALUE in lcc_pull, IP_STENCIL_VALUE_GRADIENT in Back::epilogue), the finish and the dispatch on dtype, dim and order.
// lcc_common.hpp holds what lcc_affine.hip shares with this file: Win, window_march, Stats, lcc_stats, the tiling and the workspace
// helpers.
// ===========================================================================
#include "lcc_common.hpp"                                         // Win, window_march, Stats, lcc_stats, the tiling, the workspace

namespace ip {
namespace lcc {

using namespace dt;

// ---- stage 1: I = pull(moving, disp) ---------------------------------------------------------------------------------------
template <typename R, int D, int KMAX>
__global__ __launch_bounds__(BLOCK) void lcc_pull(KParams p, const R *__restrict__ moving, const R *__restrict__ disp,
                                                  R *__restrict__ I, int B)
{
    const int64_t o = compose_sample<D>(p);
    if (o < 0) return;
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        R xr[D];
        load_coords<R, R, D>(p, disp, b, o, xr);                    // the coordinate is formed in R, as everywhere
        double x[D];
#pragma unroll
        for (int d = 0; d < D; ++d) x[d] = (double)xr[d];
        Stencil<double, D, KMAX, true, NEED_W> s;                   // ... and the weights and the sum in double: I is rounded ONCE
        s.setup(p, x);
        const R *mb = moving + b * p.vol_sb;
        R *ob = I + b * p.C * p.N + o;
        for (int c = 0; c < p.C; ++c) {
            const R *v0 = mb + c * p.vol_sc;
            opaque(s);
            double a0 = 0.0;
            IP_STENCIL_VALUE(s, v0, a0);
            ob[c * p.N] = (R)(a0 * s.mask);
        }
    }
}

// ---- stage 3: the gradient and the Hessian ----------------------------------------------------------------------------------------
template <typename R, int D, int KMAX> struct Back {
    const KParams &p;
    const double *acf; const R *I, *J, *mov, *disp; R *grad, *hess; int64_t N, b; int c, K;
    __device__ __forceinline__ Back(const KParams &p_) : p(p_) {}
    __device__ __forceinline__ double load(int q, int64_t lin) const { return acf[q * N + lin]; }
    static __device__ __forceinline__ void accumulate(const double *v, double *s)
    {
        s[0] += v[0]; s[1] += v[1]; s[2] += v[2];
    }
    static __device__ __forceinline__ void merge(double *s, const double *part) { s[0] += part[0]; s[1] += part[1]; s[2] += part[2]; }
    __device__ __forceinline__ void epilogue(int64_t o, int, const double *sum)
    {
        const R dI = (R)(-(double)J[o] * sum[0] + (double)I[o] * sum[1] + sum[2]);
        const R Cs = (R)sum[1];
        R x[D];
        load_coords<R, R, D>(p, disp, b, o, x);
        Stencil<R, D, KMAX, true, NEED_G> s;
        s.setup(p, x);
        R a0 = R(0), a1 = R(0), a2 = R(0), aw = R(0);               // (one channel per call: the offsets stay as they are; `aw` is dead code)
        IP_STENCIL_VALUE_GRADIENT(s, mov, aw, a0, a1, a2);
        const R acc[3] = { a0, a1, a2 };
        R g[D];
#pragma unroll
        for (int d = 0; d < D; ++d) g[d] = acc[d] * s.mask;
        // the channels are summed in place: this thread alone touches its sample, channel 0 stores, the others add
        R *gp = grad + o * D;
#pragma unroll
        for (int d = 0; d < D; ++d) gp[d] = c ? fma_(dI, g[d], gp[d]) : dI * g[d];
        if (K) {
            R *hp = hess + o * K;
#pragma unroll
            for (int d = 0; d < D; ++d) { const R v = Cs * g[d] * g[d]; hp[d] = c ? hp[d] + v : v; }
            if (K > D) {
#pragma unroll
                for (int d = 0; d < D; ++d) {
#pragma unroll
                    for (int e = d + 1; e < D; ++e) {
                        const int k = diag_first_index(d, e, D);
                        const R v = Cs * g[d] * g[e];
                        hp[k] = c ? hp[k] + v : v;
                    }
                }
            }
        }
    }
};

template <typename R, int D, int KMAX, int WX>
__global__ __launch_bounds__(BLOCK) void lcc_back(KParams p, Win w, const R *__restrict__ moving, const R *__restrict__ fixed,
                                                  const R *__restrict__ disp, const R *__restrict__ I, const double *__restrict__ acf,
                                                  R *gradient, R *hessian, int K, Strides sb, int B)
{
    __shared__ double raw[3][HY][HZ];
    __shared__ double tmp[3][HY][TZ];
    __shared__ double ring[WX][3][BLOCK];
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        Back<R, D, KMAX> bk(p);
        bk.N = p.N; bk.b = b; bk.K = K; bk.disp = disp;
        bk.grad = gradient + b * sb.gradient;
        bk.hess = K ? hessian + b * sb.hessian : nullptr;
        for (int c = 0; c < p.C; ++c) {
            bk.c = c;
            bk.acf = acf + (b * p.C + c) * 3 * p.N;
            bk.I = I + (b * p.C + c) * p.N;
            bk.J = fixed + b * p.val_sb + c * p.val_sc;
            bk.mov = moving + b * p.vol_sb + c * p.vol_sc;
            window_march<double, 3, 3, WX>(w, bk, raw, tmp, ring);
        }
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------
struct Args {
    KParams k; Win w; int B; int K; double eps; Strides sb;
    const void *moving, *fixed, *disp, *weight; void *loss, *gradient, *hessian; double *slots; void *I, *acf; hipStream_t st;
};

template <typename R, int D, int KMAX, int WX>
static void lcc_launch(const Args &a)
{
    const unsigned by = (unsigned)(a.B < 65535 ? a.B : 65535);
    const unsigned groups = (unsigned)lcc_groups(a.w);
    hipLaunchKernelGGL((lcc_pull<R, D, KMAX>), dim3((unsigned)pull_blocks(a.k), by, 1), dim3(BLOCK), 0, a.st, a.k, (const R *)a.moving,
                       (const R *)a.disp, (R *)a.I, a.B);
    hipLaunchKernelGGL((lcc_stats<R, WX>), dim3(groups, by, 1), dim3(BLOCK), 0, a.st, a.k, a.w, (const R *)a.I, (const R *)a.fixed,
                       (const R *)a.weight, (double *)a.acf, a.slots, a.eps, a.sb, a.B);
    hipLaunchKernelGGL((slot_finish<R>), dim3(by), dim3(BLOCK), 0, a.st, (const double *)a.slots, (R *)a.loss, (int64_t)groups, a.B, -1.0);
    hipLaunchKernelGGL((lcc_back<R, D, KMAX, WX>), dim3(groups, by, 1), dim3(BLOCK), 0, a.st, a.k, a.w, (const R *)a.moving,
                       (const R *)a.fixed, (const R *)a.disp, (const R *)a.I, (const double *)a.acf, (R *)a.gradient, (R *)a.hessian, a.K,
                       a.sb, a.B);
}

template <typename R, int D, int KMAX>
static void lcc_by_ring(const Args &a)
{
    if (D < 3) return lcc_launch<R, D, KMAX, 1>(a);                 // (no march: the lattice has one x-plane)
    if (a.w.r[0] <= 2) return lcc_launch<R, D, KMAX, (D < 3 ? 1 : 5)>(a);
    return lcc_launch<R, D, KMAX, (D < 3 ? 1 : 9)>(a);
}

} // namespace lcc
} // namespace ip

extern "C" {

int64_t interpol_lcc_workspace(const interpol_problem *p)
{
    ip::KParams k; int B; uint64_t mspan;
    const int rc = ip::dt::problem_params(p, ip::dt::LATTICE_FIELD, &k, &B, &mspan);
    if (rc) return rc;
    const int64_t groups = ip::lcc::lcc_groups(ip::lcc::lcc_tiling(k));
    if (groups > 0x7fffffffll || ip::lcc::pull_blocks(k) > 0x7fffffffll) return INTERPOL_E_SHAPE;
    return (int64_t)ip::lcc::lcc_ws_bytes(k, (uint64_t)B, groups, p->dtype == INTERPOL_F64 ? 8 : 4);
}

int interpol_lcc(const interpol_problem *p, const void *moving, const void *fixed, const void *disp, const void *weight,
                 void *loss, void *gradient, void *hessian, int hessian_kind, const int *window, double eps,
                 int64_t weight_batch_stride, int64_t gradient_batch_stride, int64_t hessian_batch_stride, void *workspace,
                 int64_t workspace_bytes, void *stream)
{
    using namespace ip::lcc;
    Args a;
    uint64_t mimage;
    const int rc = problem_params(p, LATTICE_FIELD, &a.k, &a.B, &mimage);
    if (rc) return rc;
    if (hessian_kind != HK_NONE && hessian_kind != HK_DIAG && hessian_kind != HK_FULL) return INTERPOL_E_SHAPE;
    if (!window) return INTERPOL_E_NULL;
    if (!(eps > 0.0) || !(eps < 1e300)) return INTERPOL_E_SHAPE;   // (NaN and infinity included)
    const int D = a.k.dim, K = hess_components(D, hessian_kind);
    a.w = lcc_tiling(a.k);
    for (int d = 0; d < D; ++d) {
        if (window[d] < 1 || window[d] > 2 * RMAX + 1 || window[d] % 2 == 0) return INTERPOL_E_SHAPE;
        a.w.r[3 - D + d] = (window[d] - 1) / 2;
    }
    const int64_t groups = lcc_groups(a.w);
    if (groups > 0x7fffffffll || pull_blocks(a.k) > 0x7fffffffll) return INTERPOL_E_SHAPE;
    a.K = K;
    a.eps = eps;
    const uint64_t B = (uint64_t)a.B, N = (uint64_t)a.k.N;
    const uint64_t es = p->dtype == INTERPOL_F64 ? 8 : 4;
    if (gradient_batch_stride < 0 || (weight && weight_batch_stride < 0) || (K && hessian_batch_stride < 0)) return INTERPOL_E_STRIDE;
    if (B > 1 && ((uint64_t)gradient_batch_stride < N * D || (K && (uint64_t)hessian_batch_stride < N * K))) return INTERPOL_E_STRIDE;
    if (!moving || !fixed || !disp || !loss || !gradient || !workspace || (K && !hessian)) return INTERPOL_E_NULL;
    if ((uintptr_t)workspace % sizeof(double)) return INTERPOL_E_STRIDE;             // (the slots are doubles)
    const uint64_t wsbytes = lcc_ws_bytes(a.k, B, groups, es);
    if (workspace_bytes < (int64_t)wsbytes) return INTERPOL_E_SCRATCH;
    // what is written (loss, gradient, hessian, workspace) overlaps neither an input nor each other
    const Range rd[4] = { { moving, moving_bytes(a.k, B, es, mimage) }, { fixed, fixed_bytes(a.k, B, es) },
                          { disp, ((B - 1) * (uint64_t)a.k.grid_sb + N * D) * es }, { weight, weight_bytes(a.k, B, es, weight, weight_batch_stride) } };
    const Range wr[4] = { { loss, B * es }, { gradient, ((B - 1) * (uint64_t)gradient_batch_stride + N * D) * es },
                          { hessian, K ? ((B - 1) * (uint64_t)hessian_batch_stride + N * K) * es : 0 }, { workspace, wsbytes } };
    if (ranges_alias(rd, 4, wr, 4)) return INTERPOL_E_STRIDE;
    a.sb.weight = weight ? weight_batch_stride : 0;
    a.sb.gradient = gradient_batch_stride;
    a.sb.hessian = K ? hessian_batch_stride : 0;
    a.moving = moving; a.fixed = fixed; a.disp = disp; a.weight = weight;
    a.loss = loss; a.gradient = gradient; a.hessian = K ? hessian : nullptr;
    a.slots = (double *)workspace;
    a.acf = (char *)workspace + lcc_slot_bytes(B, groups);
    a.I = (char *)a.acf + lcc_acf_bytes(a.k, B);
    a.st = (hipStream_t)stream;
    dispatch(p, a.k, [&](auto r, auto d, auto kmax) { lcc_by_ring<decltype(r), decltype(d)::value, decltype(kmax)::value>(a); });
    return hipGetLastError() == hipSuccess ? 0 : INTERPOL_E_LAUNCH;
}

} // extern "C"
