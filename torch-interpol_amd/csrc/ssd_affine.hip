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
// interpol_ssd_affine).  The accumulation of the sums (both organisations), the reduction and the finish live in affine_sums.hpp,
// which mi_affine.hip shares: the kernels here hand their per-sample terms over as a functor.  The validation of the problem
// (problem_params, LATTICE_AFFINE), the alias check, the stencil loop of one channel and the dispatch on dtype, dim and order live in
// data_term.hpp, which every data term shares.
// ===========================================================================
#include "affine_sums.hpp"                                         // the sums, their organisations, the finish; data_term.hpp

namespace ip {
namespace ssd_affine {

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
        R aw, av[3];
        stencil_value_gradient<R, D, KMAX>(p, s, v0, aw, av);
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
    sample_index<D>(p, o, od);
    lt = wt * la;
#pragma unroll
    for (int d = 0; d < D; ++d) q[d] = wt * ga[d];
    if (HESS) {
#pragma unroll
        for (int k = 0; k < K; ++k) h[k] = wt * ha[k];
    }
}

// sample_terms as the functor that the sums of affine_sums.hpp take
template <typename R, int D, int KMAX, bool HESS>
struct SsdTerms {
    const KParams &p; const R *mb, *fb, *ab, *wb;
    __device__ __forceinline__ void operator()(int64_t o, double *od, R &lt, R *q, R *h) const
    {
        sample_terms<R, D, KMAX, HESS>(p, mb, fb, ab, wb, o, od, lt, q, h);
    }
};

// moving (B, C, *in) through p.vol_sb / p.vol_sc / p.vol_ss (bytes), fixed (B, C, *shape) through p.val_sb / p.val_sc, mat
// (B, D, D+1) through mat_sb, weight (B, *shape) through weight_sb; sums (B, NS, SA_BLOCKS) doubles
template <typename R, int D, int KMAX, bool HESS>
__global__ __launch_bounds__(BLOCK) void ssd_affine_partial(KParams p, const R *__restrict__ moving, const R *__restrict__ fixed,
                                                            const R *__restrict__ mat, const R *__restrict__ weight,
                                                            double *__restrict__ sums, int64_t mat_sb, int64_t weight_sb)
{
    const int64_t b = blockIdx.y;
    const SsdTerms<R, D, KMAX, HESS> terms{ p, moving + b * p.vol_sb, fixed + b * p.val_sb, mat + b * mat_sb,
                                            weight ? weight + b * weight_sb : nullptr };
    partial_sums<R, D, HESS>(p, terms, sums, b);
}

// The staged organisation of the same sums (affine_sums.hpp: partial_sums_staged).  Which organisation serves which order:
// `staged` below.
template <typename R, int D, int KMAX>
__global__ __launch_bounds__(BLOCK) void ssd_affine_partial_staged(KParams p, const R *__restrict__ moving, const R *__restrict__ fixed,
                                                                   const R *__restrict__ mat, const R *__restrict__ weight,
                                                                   double *__restrict__ sums, int64_t mat_sb, int64_t weight_sb)
{
    const int64_t b = blockIdx.y;
    const SsdTerms<R, D, KMAX, true> terms{ p, moving + b * p.vol_sb, fixed + b * p.val_sb, mat + b * mat_sb,
                                            weight ? weight + b * weight_sb : nullptr };
    partial_sums_staged<R, D>(p, terms, sums, b);
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
    constexpr int NS = num_sums(D, HESS);
    __shared__ double tot[NS];
    const int64_t b = blockIdx.x;
    finish_sums<D, HESS>(sums, b, tot);
    if (threadIdx.x == 0) loss[b] = (R)(0.5 * tot[0]);
    write_gradient_hessian<R, D, HESS>(tot, b, gradient, hessian);
}

// ---- host side --------------------------------------------------------------------------------------------------------
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

} // namespace ssd_affine
} // namespace ip

extern "C" {

int64_t interpol_ssd_affine_workspace(const interpol_problem *p)
{
    ip::KParams k; int B; uint64_t mspan;
    const int rc = ip::dt::problem_params(p, ip::dt::LATTICE_AFFINE, &k, &B, &mspan);
    if (rc) return rc;
    return ip::ssd_affine::sa_workspace(k.dim, B);
}

int interpol_ssd_affine(const interpol_problem *p, const void *moving, const void *fixed, const void *mat, const void *weight,
                        void *loss, void *gradient, void *hessian, int with_hessian, int64_t mat_batch_stride,
                        int64_t weight_batch_stride, void *workspace, int64_t workspace_bytes, void *stream)
{
    using namespace ip::ssd_affine;
    Args a;
    uint64_t mimage;
    const int rc = problem_params(p, LATTICE_AFFINE, &a.k, &a.B, &mimage);
    if (rc) return rc;
    if (with_hessian != 0 && with_hessian != 1) return INTERPOL_E_SHAPE;
    a.hess = with_hessian != 0;
    const int D = a.k.dim;
    const uint64_t B = (uint64_t)a.B, P = (uint64_t)params(D);
    const uint64_t es = p->dtype == INTERPOL_F64 ? 8 : 4;
    if (mat_batch_stride < 0 || (weight && weight_batch_stride < 0)) return INTERPOL_E_STRIDE;
    if (!moving || !fixed || !mat || !loss || !gradient || !workspace || (a.hess && !hessian)) return INTERPOL_E_NULL;
    if ((uintptr_t)workspace % sizeof(double)) return INTERPOL_E_STRIDE;             // (the sums are doubles)
    const uint64_t wsbytes = (uint64_t)sa_workspace(D, a.B);
    if (workspace_bytes < (int64_t)wsbytes) return INTERPOL_E_SCRATCH;
    // what is written (loss, gradient, hessian, workspace) overlaps neither an input nor each other
    const Range rd[4] = { { moving, moving_bytes(a.k, B, es, mimage) }, { fixed, fixed_bytes(a.k, B, es) },
                          { mat, ((B - 1) * (uint64_t)mat_batch_stride + P) * es }, { weight, weight_bytes(a.k, B, es, weight, weight_batch_stride) } };
    const Range wr[4] = { { loss, B * es }, { gradient, B * P * es }, { hessian, a.hess ? B * P * P * es : 0 }, { workspace, wsbytes } };
    if (ranges_alias(rd, 4, wr, 4)) return INTERPOL_E_STRIDE;
    a.mat_sb = mat_batch_stride;
    a.weight_sb = weight ? weight_batch_stride : 0;
    a.moving = moving; a.fixed = fixed; a.mat = mat; a.weight = weight;
    a.loss = loss; a.gradient = gradient; a.hessian = a.hess ? hessian : nullptr;
    a.sums = (double *)workspace; a.st = (hipStream_t)stream;
    dispatch(p, a.k, [&](auto r, auto d, auto kmax) { sa_by_hessian<decltype(r), decltype(d)::value, decltype(kmax)::value>(a); });
    return hipGetLastError() == hipSuccess ? 0 : INTERPOL_E_LAUNCH;
}

} // extern "C"
