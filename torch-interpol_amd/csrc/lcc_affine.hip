// ===========================================================================
// lcc_affine.hip -- the local (windowed) normalised cross-correlation data term of a Gauss-Newton step on the matrix of an AFFINE
// lattice: the loss of lcc.hip, the gradient of the D (D+1) matrix entries and the positive part of their P x P Hessian (P = D (D+1)).
//
//     x(o) = A_b o + t_b                                         load_coords, sep == 3, from mat + b * stride (one matrix per item)
//     I, G, J, the window sums, a, c, f, A, C, F, dI             exactly as lcc.hip defines them, at x(o);   o~ = (o_0 .. o_{D-1}, 1)
//     loss[b]                                = - sum_o weight(o) sum_c cc_c(o)
//     gradient[b, d, e]                      = sum_o sum_c dI_c(o) G_cd(o) o~_e
//     hessian[b, d (D+1) + e, d' (D+1) + e'] = sum_o sum_c C_c(o) G_cd(o) G_cd'(o) o~_e o~_e'
//
// Five stages on the caller's stream, one C call, every kernel with the item on gridDim.y (clamped) and a loop over the batch:
//   lcc_affine_pull<R, D, KMAX>  : lcc_pull of lcc.hip on the affine branch of load_coords (lcc_pull hands `b` to load_coords, which
//                                  the affine branch does not read: one matrix per item needs the pointer of the item); writes I.
//   lcc_stats<R, WX>, slot_finish<R> : unchanged (lcc_common.hpp, data_term.hpp); write a, c, f and the loss.
//   lcc_affine_march<R, WX>      : the window sums of a, c, f (double) as lcc_back forms them; the epilogue rounds dI and C to R once
//                                  and stores them per sample and channel: (B, C, 2, N) of R in the workspace.  No stencil, no
//                                  gradient or Hessian field: the stencil's registers are out of the march.
//   lcc_affine_partial<R, D, KMAX, HESS> / lcc_affine_partial_staged<R, D, KMAX> : the sums of affine_sums.hpp with ONE
//                                  Stencil<R, D, KMAX, true, NEED_G> per sample for all channels: q_d = sum_c dI_c G_cd and h_dd' =
//                                  sum_c C_c G_cd G_cd' in R, each converted to double once; the loss term is 0 (the loss is stage 2's).
//   lcc_affine_finish<R, D, HESS>: finish_sums and write_gradient_hessian per item; does not touch `loss`.
//
// No atomics, nothing in the workspace is assumed cleared: two calls give identical bits, an item gives the same bits alone or
// inside a batch, and the launches replay from a captured graph.  Stages 3 and 4 are NOT fused: the 73 accumulators of the sums on
// top of the march's registers and 83 KiB of LDS would leave one workgroup per CU.  Instantiated for float / double, D = 1..3, one
// order 1..3, with and without the Hessian, rings of 1 (D < 3), 5 and 9 planes.  The C entry points live here as well
// (include/interpol_hip.h: interpol_lcc_affine_workspace, interpol_lcc_affine).
// ===========================================================================
#include "lcc_common.hpp"                                          // Win, window_march, lcc_stats, the tiling, the workspace helpers
#include "affine_sums.hpp"                                         // the sums, their organisations, the finish

namespace ip {
namespace lcc_affine {

using namespace ip::lcc;
using namespace ip::ssd_affine;

// ---- stage 1: I = pull(moving, A o + t) --------------------------------------------------------------------------------------
template <typename R, int D, int KMAX>
__global__ __launch_bounds__(BLOCK) void lcc_affine_pull(KParams p, const R *__restrict__ moving, const R *__restrict__ mat,
                                                         R *__restrict__ I, int64_t mat_sb, int B)
{
    const int64_t o = compose_sample<D>(p);
    if (o < 0) return;
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        R xr[D];
        load_coords<R, R, D>(p, mat + b * mat_sb, 0, o, xr);        // the coordinate is formed in R, as everywhere
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

// ---- stage 3: dI and C per sample and channel --------------------------------------------------------------------------------
// the window sums of lcc.hip's Back with its epilogue cut after dI and C
template <typename R> struct Mid {
    const double *acf; const R *I, *J; R *dic; int64_t N;
    __device__ __forceinline__ double load(int q, int64_t lin) const { return acf[q * N + lin]; }
    static __device__ __forceinline__ void accumulate(const double *v, double *s)
    {
        s[0] += v[0]; s[1] += v[1]; s[2] += v[2];
    }
    static __device__ __forceinline__ void merge(double *s, const double *part) { s[0] += part[0]; s[1] += part[1]; s[2] += part[2]; }
    __device__ __forceinline__ void epilogue(int64_t o, int, const double *sum)
    {
        dic[o] = (R)(-(double)J[o] * sum[0] + (double)I[o] * sum[1] + sum[2]);
        dic[N + o] = (R)sum[1];
    }
};

// I (B, C, N), fixed through p.val_sb / p.val_sc, acf (B, C, 3, N) -> dic (B, C, 2, N)
template <typename R, int WX>
__global__ __launch_bounds__(BLOCK) void lcc_affine_march(KParams p, Win w, const R *__restrict__ fixed, const R *__restrict__ I,
                                                          const double *__restrict__ acf, R *__restrict__ dic, int B)
{
    __shared__ double raw[3][HY][HZ];
    __shared__ double tmp[3][HY][TZ];
    __shared__ double ring[WX][3][BLOCK];
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        Mid<R> md;
        md.N = p.N;
        for (int c = 0; c < p.C; ++c) {
            md.acf = acf + (b * p.C + c) * 3 * p.N;
            md.I = I + (b * p.C + c) * p.N;
            md.J = fixed + b * p.val_sb + c * p.val_sc;
            md.dic = dic + (b * p.C + c) * 2 * p.N;
            window_march<double, 3, 3, WX>(w, md, raw, tmp, ring);
        }
    }
}

// ---- stage 4: the sums of the gradient and of the Hessian ----------------------------------------------------------------------
// the per-sample terms as the functor that the sums of affine_sums.hpp take: one stencil for every channel; db = the item's (C, 2, N)
template <typename R, int D, int KMAX, bool HESS>
struct LccTerms {
    const KParams &p; const R *mb, *ab, *db;
    __device__ __forceinline__ void operator()(int64_t o, double *od, R &lt, R *q, R *h) const
    {
        constexpr int K = D * (D + 1) / 2;
        R x[D];
        load_coords<R, R, D>(p, ab, 0, o, x);
        Stencil<R, D, KMAX, true, NEED_G> s;
        s.setup(p, x);
#pragma unroll
        for (int d = 0; d < D; ++d) q[d] = R(0);
        if (HESS) {
#pragma unroll
            for (int k = 0; k < K; ++k) h[k] = R(0);
        }
        for (int c = 0; c < p.C; ++c) {
            R aw, av[3];
            stencil_value_gradient<R, D, KMAX>(p, s, mb + c * p.vol_sc, aw, av);
            const R dI = db[(int64_t)c * 2 * p.N + o], Cs = db[((int64_t)c * 2 + 1) * p.N + o];
            R g[D];
#pragma unroll
            for (int d = 0; d < D; ++d) g[d] = av[d] * s.mask;
#pragma unroll
            for (int d = 0; d < D; ++d) q[d] = fma_(dI, g[d], q[d]);
            if (HESS) {
#pragma unroll
                for (int d = 0; d < D; ++d) {
#pragma unroll
                    for (int e = d; e < D; ++e) h[pair_index(d, e, D)] = fma_(Cs * g[d], g[e], h[pair_index(d, e, D)]);
                }
            }
        }
        sample_index<D>(p, o, od);
        lt = R(0);
    }
};

// moving (B, C, *in) through p.vol_sb / p.vol_sc / p.vol_ss, mat (B, D, D+1) through mat_sb, dic (B, C, 2, N); sums (B, NS, SA_BLOCKS)
// doubles.  (partial_sums ends with threads that read its shared rows: the barrier keeps the next item's writes behind them.)
template <typename R, int D, int KMAX, bool HESS>
__global__ __launch_bounds__(BLOCK) void lcc_affine_partial(KParams p, const R *__restrict__ moving, const R *__restrict__ mat,
                                                            const R *__restrict__ dic, double *__restrict__ sums, int64_t mat_sb, int B)
{
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        const LccTerms<R, D, KMAX, HESS> terms{ p, moving + b * p.vol_sb, mat + b * mat_sb, dic + b * p.C * 2 * p.N };
        partial_sums<R, D, HESS>(p, terms, sums, b);
        __syncthreads();
    }
}

// The staged organisation of the same sums (affine_sums.hpp: partial_sums_staged).  Which organisation serves which order: `staged`.
template <typename R, int D, int KMAX>
__global__ __launch_bounds__(BLOCK) void lcc_affine_partial_staged(KParams p, const R *__restrict__ moving, const R *__restrict__ mat,
                                                                   const R *__restrict__ dic, double *__restrict__ sums, int64_t mat_sb,
                                                                   int B)
{
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        const LccTerms<R, D, KMAX, true> terms{ p, moving + b * p.vol_sb, mat + b * mat_sb, dic + b * p.C * 2 * p.N };
        partial_sums_staged<R, D>(p, terms, sums, b);
        __syncthreads();
    }
}

// The choice of ssd_affine.hip: the per-sample term is its residual's with two loads in place of one.
constexpr bool staged(int D, int KMAX, bool hess) { return hess && D == 3 && KMAX == 3; }

// sums (B, NS, SA_BLOCKS) doubles -> gradient (B, D, D+1), hessian (B, P, P); one workgroup per item
template <typename R, int D, bool HESS>
__global__ __launch_bounds__(BLOCK) void lcc_affine_finish(const double *__restrict__ sums, R *__restrict__ gradient, R *__restrict__ hessian)
{
    constexpr int NS = num_sums(D, HESS);
    __shared__ double tot[NS];
    const int64_t b = blockIdx.x;
    finish_sums<D, HESS>(sums, b, tot);
    write_gradient_hessian<R, D, HESS>(tot, b, gradient, hessian);
}

// ---- host side --------------------------------------------------------------------------------------------------------
struct Args {
    KParams k; Win w; int B; bool hess; double eps; int64_t mat_sb; Strides sb;
    const void *moving, *fixed, *mat, *weight; void *loss, *gradient, *hessian; double *slots, *acf, *sums; void *I, *dic; hipStream_t st;
};

// the workspace: the slots (B, groups), a, c, f (B, C, 3, N) and the sums (B, NS, SA_BLOCKS), doubles, then I (B, C, N) and dI, C
// (B, C, 2, N) of the dtype
static uint64_t image_bytes(const KParams &k, uint64_t B, uint64_t es) { return (B * (uint64_t)k.C * (uint64_t)k.N * es + 7) & ~(uint64_t)7; }
static uint64_t la_ws_bytes(const KParams &k, uint64_t B, int64_t groups, uint64_t es)
{
    return lcc_slot_bytes(B, groups) + lcc_acf_bytes(k, B) + (uint64_t)sa_workspace(k.dim, (int)B) + image_bytes(k, B, es) + image_bytes(k, 2 * B, es);
}

template <typename R, int D, int KMAX, int WX, bool HESS>
static void la_launch(const Args &a)
{
    const unsigned by = (unsigned)(a.B < 65535 ? a.B : 65535);
    const unsigned groups = (unsigned)lcc_groups(a.w);
    hipLaunchKernelGGL((lcc_affine_pull<R, D, KMAX>), dim3((unsigned)pull_blocks(a.k), by, 1), dim3(BLOCK), 0, a.st, a.k,
                       (const R *)a.moving, (const R *)a.mat, (R *)a.I, a.mat_sb, a.B);
    hipLaunchKernelGGL((lcc_stats<R, WX>), dim3(groups, by, 1), dim3(BLOCK), 0, a.st, a.k, a.w, (const R *)a.I, (const R *)a.fixed,
                       (const R *)a.weight, a.acf, a.slots, a.eps, a.sb, a.B);
    hipLaunchKernelGGL((slot_finish<R>), dim3(by), dim3(BLOCK), 0, a.st, (const double *)a.slots, (R *)a.loss, (int64_t)groups, a.B, -1.0);
    hipLaunchKernelGGL((lcc_affine_march<R, WX>), dim3(groups, by, 1), dim3(BLOCK), 0, a.st, a.k, a.w, (const R *)a.fixed,
                       (const R *)a.I, (const double *)a.acf, (R *)a.dic, a.B);
    if constexpr (staged(D, KMAX, HESS))
        hipLaunchKernelGGL((lcc_affine_partial_staged<R, D, KMAX>), dim3(SA_BLOCKS, by, 1), dim3(BLOCK), 0, a.st, a.k, (const R *)a.moving,
                           (const R *)a.mat, (const R *)a.dic, a.sums, a.mat_sb, a.B);
    else
        hipLaunchKernelGGL((lcc_affine_partial<R, D, KMAX, HESS>), dim3(SA_BLOCKS, by, 1), dim3(BLOCK), 0, a.st, a.k, (const R *)a.moving,
                           (const R *)a.mat, (const R *)a.dic, a.sums, a.mat_sb, a.B);
    hipLaunchKernelGGL((lcc_affine_finish<R, D, HESS>), dim3((unsigned)a.B), dim3(BLOCK), 0, a.st, (const double *)a.sums,
                       (R *)a.gradient, (R *)a.hessian);
}

template <typename R, int D, int KMAX, int WX>
static void la_by_hessian(const Args &a)
{
    if (a.hess) la_launch<R, D, KMAX, WX, true>(a);
    else la_launch<R, D, KMAX, WX, false>(a);
}

template <typename R, int D, int KMAX>
static void la_by_ring(const Args &a)
{
    if (D < 3) return la_by_hessian<R, D, KMAX, 1>(a);              // (no march: the lattice has one x-plane)
    if (a.w.r[0] <= 2) return la_by_hessian<R, D, KMAX, (D < 3 ? 1 : 5)>(a);
    return la_by_hessian<R, D, KMAX, (D < 3 ? 1 : 9)>(a);
}

} // namespace lcc_affine
} // namespace ip

extern "C" {

int64_t interpol_lcc_affine_workspace(const interpol_problem *p)
{
    ip::KParams k; int B; uint64_t mspan;
    const int rc = ip::dt::problem_params(p, ip::dt::LATTICE_AFFINE_LOOPED, &k, &B, &mspan);
    if (rc) return rc;
    const int64_t groups = ip::lcc::lcc_groups(ip::lcc::lcc_tiling(k));
    if (groups > 0x7fffffffll || ip::lcc::pull_blocks(k) > 0x7fffffffll) return INTERPOL_E_SHAPE;
    return (int64_t)ip::lcc_affine::la_ws_bytes(k, (uint64_t)B, groups, p->dtype == INTERPOL_F64 ? 8 : 4);
}

int interpol_lcc_affine(const interpol_problem *p, const void *moving, const void *fixed, const void *mat, const void *weight,
                        void *loss, void *gradient, void *hessian, int with_hessian, const int *window, double eps,
                        int64_t mat_batch_stride, int64_t weight_batch_stride, void *workspace, int64_t workspace_bytes, void *stream)
{
    using namespace ip::lcc_affine;
    Args a;
    uint64_t mimage;
    const int rc = problem_params(p, LATTICE_AFFINE_LOOPED, &a.k, &a.B, &mimage);
    if (rc) return rc;
    if (with_hessian != 0 && with_hessian != 1) return INTERPOL_E_SHAPE;
    if (!window) return INTERPOL_E_NULL;
    if (!(eps > 0.0) || !(eps < 1e300)) return INTERPOL_E_SHAPE;   // (NaN and infinity included)
    a.hess = with_hessian != 0;
    a.eps = eps;
    const int D = a.k.dim;
    a.w = lcc_tiling(a.k);
    for (int d = 0; d < D; ++d) {
        if (window[d] < 1 || window[d] > 2 * RMAX + 1 || window[d] % 2 == 0) return INTERPOL_E_SHAPE;
        a.w.r[3 - D + d] = (window[d] - 1) / 2;
    }
    const int64_t groups = lcc_groups(a.w);
    if (groups > 0x7fffffffll || pull_blocks(a.k) > 0x7fffffffll) return INTERPOL_E_SHAPE;
    const uint64_t B = (uint64_t)a.B, P = (uint64_t)params(D);
    const uint64_t es = p->dtype == INTERPOL_F64 ? 8 : 4;
    if (mat_batch_stride < 0 || (weight && weight_batch_stride < 0)) return INTERPOL_E_STRIDE;
    if (!moving || !fixed || !mat || !loss || !gradient || !workspace || (a.hess && !hessian)) return INTERPOL_E_NULL;
    if ((uintptr_t)workspace % sizeof(double)) return INTERPOL_E_STRIDE;             // (the slots are doubles)
    const uint64_t wsbytes = la_ws_bytes(a.k, B, groups, es);
    if (workspace_bytes < (int64_t)wsbytes) return INTERPOL_E_SCRATCH;
    // what is written (loss, gradient, hessian, workspace) overlaps neither an input nor each other
    const Range rd[4] = { { moving, moving_bytes(a.k, B, es, mimage) }, { fixed, fixed_bytes(a.k, B, es) },
                          { mat, ((B - 1) * (uint64_t)mat_batch_stride + P) * es }, { weight, weight_bytes(a.k, B, es, weight, weight_batch_stride) } };
    const Range wr[4] = { { loss, B * es }, { gradient, B * P * es }, { hessian, a.hess ? B * P * P * es : 0 }, { workspace, wsbytes } };
    if (ranges_alias(rd, 4, wr, 4)) return INTERPOL_E_STRIDE;
    a.mat_sb = mat_batch_stride;
    a.sb.weight = weight ? weight_batch_stride : 0;
    a.sb.gradient = 0; a.sb.hessian = 0;                            // (lcc_stats reads the weight's stride alone)
    a.moving = moving; a.fixed = fixed; a.mat = mat; a.weight = weight;
    a.loss = loss; a.gradient = gradient; a.hessian = a.hess ? hessian : nullptr;
    char *ws = (char *)workspace;
    a.slots = (double *)ws;                    ws += lcc_slot_bytes(B, groups);
    a.acf = (double *)ws;                      ws += lcc_acf_bytes(a.k, B);
    a.sums = (double *)ws;                     ws += sa_workspace(D, a.B);
    a.I = ws;                                  ws += image_bytes(a.k, B, es);
    a.dic = ws;
    a.st = (hipStream_t)stream;
    dispatch(p, a.k, [&](auto r, auto d, auto kmax) { la_by_ring<decltype(r), decltype(d)::value, decltype(kmax)::value>(a); });
    return hipGetLastError() == hipSuccess ? 0 : INTERPOL_E_LAUNCH;
}

} // extern "C"
