// ===========================================================================
// mi_affine.hip -- the mutual-information data term of a step on the matrix of an AFFINE lattice: loss, gradient of the D (D+1)
// matrix entries and a P x P majoriser of their Hessian (P = D (D+1)), one channel.  Three stages on one stream, one C call.
//
//     x(o) = A_b o + t_b,   I = mask(x) pull(moving, x),   G_d = mask(x) grad_d(moving, x),   J = fixed(o),   omega = weight mask
//     t_m = clamp((I - m_lo) m_sc, 0, 1),  u = 1.5 + t_m (B - 4),  taps j = floor(u) - 1 .. floor(u) + 2 with the cubic B-spline
//     t_f = clamp((J - f_lo) f_sc, 0, 1),  k = floor(t_f (B - 1) + 1/2)
//     P[j, k] = sum_o omega beta3(u - j) [k = k(o)] / W,   p_m = sum_k P,  p_f = sum_j P,  T = log(P / (p_m p_f)) (0 where P = 0)
//     loss = - sum P T
//     dI = -(omega / W) s sum_j beta3'(u - j) T[j, k],   c = (omega / W) s^2 sum_j |beta3''(u - j)| |T[j, k]|,   s = (B - 4) m_sc
//     (s = 0 for a sample whose t_m was clamped);   q_d = dI G_d,   h_dd' = c G_d G_d'   into the sums of affine_sums.hpp.
//
//   mi_histogram<R, D, KMAX> : MI_BLOCKS persistent workgroups per item.  Per sample the affine branch of load_coords in R and ONE
//       Stencil, evaluated in DOUBLE from the tensors' values together with u, k and beta3 (sample_value_double: the tap weight
//       at the end of the spline's support is ill-conditioned in u); four fixed-point updates (ds_add_u64) into a B x B histogram of
//       64-bit integers in LDS; the non-zero bins go to the item's histogram in the workspace with 64-bit integer atomics.
//       The quantum is q = wmax 2^-shift, shift = min(52, 62 - ceil(log2 N)), wmax = max|weight| of the item: an update is
//       llrint(omega beta / q) <= 2^52, N of them stay below 2^62.  Integer sums are exact in any order: the histogram does not
//       depend on the run, on the number of workgroups or on the batch the item sits in.
//   mi_table<R>              : one workgroup per item.  Row, column and total sums of the integers (exact), then P, p_m, p_f, T and
//       the loss in double; the loss terms are added in a fixed order.  Writes T rounded once to R and 1 / W into the workspace,
//       the loss and the optional histogram P.  A total <= 0 (W = 0) gives T = 0, 1 / W = 0, loss = 0: every output is zero.
//   mi_affine_partial<R, D, KMAX, HESS> / mi_affine_partial_staged<R, D, KMAX> : the sums of ssd_affine_partial with q_d = dI G_d
//       and h_dd' = c G_d G_d', T staged in LDS; the stencil is recomputed (nothing of size N is written).
//   mi_affine_finish<R, D, HESS> : the finish of ssd_affine.hip without the loss.
//
// The histogram region of the workspace is cleared by a kernel of its own in front of the first stage (mi_clear; with a memset
// node in its place the replay of a captured graph stopped matching eager at the second replay); nothing else is assumed cleared.
// No floating-point atomics: two calls give identical bits, an item gives the same bits alone or inside a batch, and the launches
// replay from a captured graph to the bits of eager.  Instantiated for float / double, D = 1..3, one order 1..3, with and
// without the Hessian, 8 <= B <= 64 (a run-time value: the LDS of the histogram and of T is sized at launch).
// ===========================================================================
// The sums, their organisations and the finish live in affine_sums.hpp; the validation of the problem (problem_params, which
// mi_params wraps), the alias check, the stencil loops of one channel (stencil_value_gradient in sample_image, IP_STENCIL_VALUE in
// sample_value_double) and the dispatch on dtype, dim and order live in data_term.hpp; what does not care about the kind of lattice
// (the bins of a sample, the cubic B-spline, the quantum, mi_clear, mi_table, stage_table) lives in mi_common.hpp, shared with mi.hip.
#include "affine_sums.hpp"
#include "mi_common.hpp"

namespace ip {
namespace mi_affine {

using namespace ip::ssd_affine;
using namespace ip::mi;

// I, G and omega of sample o in R: the affine branch of load_coords from `ab` and one stencil
template <typename R, int D, int KMAX>
__device__ __forceinline__ void sample_image(const KParams &p, const R *mb, const R *ab, const R *wb, int64_t o, R &I, R *G, R &omega)
{
    R x[D];
    load_coords<R, R, D>(p, ab, 0, o, x);
    Stencil<R, D, KMAX, true, NEED_G> s;
    s.setup(p, x);
    const R wt = wb ? wb[o] : R(1);
    R aw, av[3];
    stencil_value_gradient<R, D, KMAX>(p, s, mb, aw, av);
    I = aw * s.mask;
#pragma unroll
    for (int d = 0; d < D; ++d) G[d] = av[d] * s.mask;
    omega = wt * s.mask;
}

// I and omega of sample o in DOUBLE from the tensors' values, for the histogram: the coordinate as load_coords forms it in R, then the
// stencil weights, the taps' sum and the mask in double.  The weight of a tap at the end of the B-spline's support, e^3 / 6 at a
// distance e inside it, has the relative sensitivity 3 / e to u: a float32 rounding of I moves a nearly empty bin by 1e-2 of
// itself, and T = log(P / (p_m p_f)) reads P relatively.
template <typename R, int D, int KMAX>
__device__ __forceinline__ void sample_value_double(const KParams &p, const R *mb, const R *ab, const R *wb, int64_t o, double &I,
                                                    double &omega)
{
    double x[D];
    load_coords<double, R, D>(p, ab, 0, o, x);
    Stencil<double, D, KMAX, true, NEED_W> s;
    s.setup(p, x);
    const double wt = wb ? (double)wb[o] : 1.0;
    opaque(s);
    double aw = 0.0;
    IP_STENCIL_VALUE(s, mb, aw);
    I = aw * s.mask;
    omega = wt * s.mask;
}

// hist (B, bins, bins) of 64-bit integers, cleared by mi_clear before the launch; ranges (B, RANGE_STRIDE) doubles
template <typename R, int D, int KMAX>
__global__ __launch_bounds__(BLOCK) void mi_histogram(KParams p, const R *__restrict__ moving, const R *__restrict__ fixed,
                                                      const R *__restrict__ mat, const R *__restrict__ weight,
                                                      const double *__restrict__ ranges, unsigned long long *__restrict__ hist,
                                                      int64_t mat_sb, int64_t weight_sb, int bins, int shift)
{
    extern __shared__ unsigned long long lh[];                      // bins x bins
    const int64_t b = blockIdx.y;
    const R *mb = moving + b * p.vol_sb;
    const R *fb = fixed + b * p.val_sb;
    const R *ab = mat + b * mat_sb;
    const R *wb = weight ? weight + b * weight_sb : nullptr;
    const double *rg = ranges + b * RANGE_STRIDE;
    const double m_lo = rg[0], m_sc = rg[1], f_lo = rg[2], f_sc = rg[3];
    const double wmax = rg[4];
    const double inv_q = wmax > 0.0 ? ldexp(1.0, shift) / wmax : 0.0;
    const int nb = bins * bins;
    for (int i = threadIdx.x; i < nb; i += BLOCK) lh[i] = 0ull;
    __syncthreads();
    for (int64_t o = (int64_t)blockIdx.x * BLOCK + threadIdx.x; o < p.N; o += (int64_t)MI_BLOCKS * BLOCK) {
        double I, omega;
        sample_value_double<R, D, KMAX>(p, mb, ab, wb, o, I, omega);
        const Bins<double> s = sample_bins<double>(I, (double)fb[o], m_lo, m_sc, f_lo, f_sc, bins);
        double w[4];
        bspline3<double>(s.f, w);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long long v = __double2ll_rn((omega * w[i]) * inv_q);
            if (v) atomicAdd(&lh[(s.j0 + i) * bins + s.k], (unsigned long long)v);       // ds_add_u64; 0 <= j0 + i < bins, 0 <= k < bins
        }
    }
    __syncthreads();
    unsigned long long *hb = hist + b * nb;
    for (int i = threadIdx.x; i < nb; i += BLOCK) {
        const unsigned long long v = lh[i];
        if (v) __hip_atomic_fetch_add(hb + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- stage 3: the sums of the gradient and of the majoriser ------------------------------------------------------------
// the per-sample terms as the functor that the sums of affine_sums.hpp take; T (bins x bins) in LDS
template <typename R, int D, int KMAX, bool HESS>
struct MiTerms {
    const KParams &p; const R *mb, *fb, *ab, *wb, *T;
    R m_lo, m_sc, f_lo, f_sc, inv_w; int bins;
    __device__ __forceinline__ void operator()(int64_t o, double *od, R &lt, R *q, R *h) const
    {
        R I, G[D], omega;
        sample_image<R, D, KMAX>(p, mb, ab, wb, o, I, G, omega);
        const Bins<R> s = sample_bins<R>(I, fb[o], m_lo, m_sc, f_lo, f_sc, bins);
        R d1[4], d2[4];
        bspline3_d1<R>(s.f, d1);
        if (HESS) bspline3_abs_d2<R>(s.f, d2);
        R a = R(0), c = R(0);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const R t = T[(s.j0 + i) * bins + s.k];
            a = fma_(d1[i], t, a);
            if (HESS) c = fma_(d2[i], fabs(t), c);
        }
        const R sc = s.clamped ? R(0) : (R)(bins - 4) * m_sc;
        const R wn = omega * inv_w;
        const R dI = -(wn * sc) * a;
        const R cc = (wn * sc) * sc * c;
        sample_index<D>(p, o, od);
        lt = R(0);
#pragma unroll
        for (int d = 0; d < D; ++d) q[d] = dI * G[d];
        if (HESS) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
#pragma unroll
                for (int e = d; e < D; ++e) h[pair_index(d, e, D)] = cc * G[d] * G[e];
            }
        }
    }
};

template <typename R, int D, int KMAX, bool HESS>
__global__ __launch_bounds__(BLOCK) void mi_affine_partial(KParams p, const R *__restrict__ moving, const R *__restrict__ fixed,
                                                           const R *__restrict__ mat, const R *__restrict__ weight,
                                                           const double *__restrict__ ranges, const R *__restrict__ table,
                                                           const double *__restrict__ inv_w, double *__restrict__ sums,
                                                           int64_t mat_sb, int64_t weight_sb, int bins)
{
    const int64_t b = blockIdx.y;
    const R *T = stage_table<R>(table, b, bins);
    const double *rg = ranges + b * RANGE_STRIDE;
    const MiTerms<R, D, KMAX, HESS> terms{ p, moving + b * p.vol_sb, fixed + b * p.val_sb, mat + b * mat_sb,
                                           weight ? weight + b * weight_sb : nullptr, T,
                                           (R)rg[0], (R)rg[1], (R)rg[2], (R)rg[3], (R)inv_w[b], bins };
    partial_sums<R, D, HESS>(p, terms, sums, b);
}

template <typename R, int D, int KMAX>
__global__ __launch_bounds__(BLOCK) void mi_affine_partial_staged(KParams p, const R *__restrict__ moving, const R *__restrict__ fixed,
                                                                  const R *__restrict__ mat, const R *__restrict__ weight,
                                                                  const double *__restrict__ ranges, const R *__restrict__ table,
                                                                  const double *__restrict__ inv_w, double *__restrict__ sums,
                                                                  int64_t mat_sb, int64_t weight_sb, int bins)
{
    const int64_t b = blockIdx.y;
    const R *T = stage_table<R>(table, b, bins);
    const double *rg = ranges + b * RANGE_STRIDE;
    const MiTerms<R, D, KMAX, true> terms{ p, moving + b * p.vol_sb, fixed + b * p.val_sb, mat + b * mat_sb,
                                           weight ? weight + b * weight_sb : nullptr, T,
                                           (R)rg[0], (R)rg[1], (R)rg[2], (R)rg[3], (R)inv_w[b], bins };
    partial_sums_staged<R, D>(p, terms, sums, b);
}

// The 3-D sums with a Hessian leave one wave per SIMD with their 73 accumulators in registers, whatever the order of the stencil
// (ssd_affine.hip: `staged`); here the term of a sample is heavier than the residual of the sum of squares, so all three orders
// take the staged organisation in 3-D with a Hessian.
constexpr bool staged(int D, int KMAX, bool hess) { return hess && D == 3; }

// sums (B, NS, SA_BLOCKS) doubles -> gradient (B, D, D+1), hessian (B, P, P)
template <typename R, int D, bool HESS>
__global__ __launch_bounds__(BLOCK) void mi_affine_finish(const double *__restrict__ sums, R *__restrict__ gradient, R *__restrict__ hessian)
{
    constexpr int NS = num_sums(D, HESS);
    __shared__ double tot[NS];
    const int64_t b = blockIdx.x;
    finish_sums<D, HESS>(sums, b, tot);
    write_gradient_hessian<R, D, HESS>(tot, b, gradient, hessian);
}

// ---- host side --------------------------------------------------------------------------------------------------------
struct Args {
    KParams k; int B; bool hess; int bins, shift; int64_t mat_sb, weight_sb;
    const void *moving, *fixed, *mat, *weight; const double *ranges; void *loss, *gradient, *hessian, *histogram;
    unsigned long long *hist; void *table; double *inv_w, *sums; hipStream_t st;
};

// the workspace: the integer histograms, T (8 bytes per entry reserved), 1 / W, the sums
static int64_t mi_workspace(int D, int B, int bins) { return 2 * hist_bytes(B, bins) + invw_bytes(B) + sa_workspace(D, B); }

template <typename R, int D, int KMAX, bool HESS>
static void mi_launch(const Args &a)
{
    const unsigned nb = (unsigned)(a.bins * a.bins);
    const dim3 items(SA_BLOCKS, (unsigned)a.B, 1);
    hipLaunchKernelGGL((mi_histogram<R, D, KMAX>), dim3(MI_BLOCKS, (unsigned)a.B, 1), dim3(BLOCK), nb * 8, a.st, a.k,
                       (const R *)a.moving, (const R *)a.fixed, (const R *)a.mat, (const R *)a.weight, a.ranges, a.hist, a.mat_sb,
                       a.weight_sb, a.bins, a.shift);
    hipLaunchKernelGGL((mi_table<R>), dim3((unsigned)a.B), dim3(BLOCK), 0, a.st, (const long long *)a.hist, a.ranges, (R *)a.table,
                       a.inv_w, (R *)a.loss, (R *)a.histogram, a.bins, a.shift);
    if constexpr (staged(D, KMAX, HESS))
        hipLaunchKernelGGL((mi_affine_partial_staged<R, D, KMAX>), items, dim3(BLOCK), nb * sizeof(R), a.st, a.k, (const R *)a.moving,
                           (const R *)a.fixed, (const R *)a.mat, (const R *)a.weight, a.ranges, (const R *)a.table,
                           (const double *)a.inv_w, a.sums, a.mat_sb, a.weight_sb, a.bins);
    else
        hipLaunchKernelGGL((mi_affine_partial<R, D, KMAX, HESS>), items, dim3(BLOCK), nb * sizeof(R), a.st, a.k, (const R *)a.moving,
                           (const R *)a.fixed, (const R *)a.mat, (const R *)a.weight, a.ranges, (const R *)a.table,
                           (const double *)a.inv_w, a.sums, a.mat_sb, a.weight_sb, a.bins);
    hipLaunchKernelGGL((mi_affine_finish<R, D, HESS>), dim3((unsigned)a.B), dim3(BLOCK), 0, a.st, (const double *)a.sums,
                       (R *)a.gradient, (R *)a.hessian);
}

template <typename R, int D, int KMAX>
static void mi_by_hessian(const Args &a)
{
    if (a.hess) mi_launch<R, D, KMAX, true>(a);
    else mi_launch<R, D, KMAX, false>(a);
}

// the problem of interpol_ssd_affine with one channel, and the bins
static int mi_params(const interpol_problem *p, int bins, KParams *k, int *B, uint64_t *mspan)
{
    const int rc = problem_params(p, LATTICE_AFFINE, k, B, mspan);
    if (rc) return rc;
    if (k->C != 1) return INTERPOL_E_SHAPE;
    if (bins < MIN_BINS || bins > MAX_BINS) return INTERPOL_E_SHAPE;
    return 0;
}

} // namespace mi_affine
} // namespace ip

extern "C" {

int64_t interpol_mi_affine_workspace(const interpol_problem *p, int bins)
{
    ip::KParams k; int B; uint64_t mspan;
    const int rc = ip::mi_affine::mi_params(p, bins, &k, &B, &mspan);
    if (rc) return rc;
    return ip::mi_affine::mi_workspace(k.dim, B, bins);
}

int interpol_mi_affine(const interpol_problem *p, const void *moving, const void *fixed, const void *mat, const void *weight,
                       const void *ranges, void *loss, void *gradient, void *hessian, void *histogram, int with_hessian, int bins,
                       int64_t mat_batch_stride, int64_t weight_batch_stride, void *workspace, int64_t workspace_bytes, void *stream)
{
    using namespace ip::mi_affine;
    Args a;
    uint64_t mimage;
    const int rc = mi_params(p, bins, &a.k, &a.B, &mimage);
    if (rc) return rc;
    if (with_hessian != 0 && with_hessian != 1) return INTERPOL_E_SHAPE;
    a.hess = with_hessian != 0;
    a.bins = bins;
    const int D = a.k.dim;
    const uint64_t B = (uint64_t)a.B, P = (uint64_t)params(D), NB = (uint64_t)bins * (uint64_t)bins;
    const uint64_t es = p->dtype == INTERPOL_F64 ? 8 : 4;
    if (mat_batch_stride < 0 || (weight && weight_batch_stride < 0)) return INTERPOL_E_STRIDE;
    if (!moving || !fixed || !mat || !ranges || !loss || !gradient || !workspace || (a.hess && !hessian)) return INTERPOL_E_NULL;
    if ((uintptr_t)workspace % sizeof(double) || (uintptr_t)ranges % sizeof(double)) return INTERPOL_E_STRIDE;   // (doubles)
    const uint64_t wsbytes = (uint64_t)mi_workspace(D, a.B, bins);
    if (workspace_bytes < (int64_t)wsbytes) return INTERPOL_E_SCRATCH;
    // what is written (loss, gradient, hessian, histogram, workspace) overlaps neither an input nor each other
    const Range rd[5] = { { moving, moving_bytes(a.k, B, es, mimage) }, { fixed, fixed_bytes(a.k, B, es) },
                          { mat, ((B - 1) * (uint64_t)mat_batch_stride + P) * es }, { weight, weight_bytes(a.k, B, es, weight, weight_batch_stride) },
                          { ranges, B * RANGE_STRIDE * sizeof(double) } };
    const Range wr[5] = { { loss, B * es }, { gradient, B * P * es }, { hessian, a.hess ? B * P * P * es : 0 },
                          { histogram, histogram ? B * NB * es : 0 }, { workspace, wsbytes } };
    if (ranges_alias(rd, 5, wr, 5)) return INTERPOL_E_STRIDE;
    a.shift = quantum_shift(a.k.N);
    a.mat_sb = mat_batch_stride;
    a.weight_sb = weight ? weight_batch_stride : 0;
    a.moving = moving; a.fixed = fixed; a.mat = mat; a.weight = weight; a.ranges = (const double *)ranges;
    a.loss = loss; a.gradient = gradient; a.hessian = a.hess ? hessian : nullptr; a.histogram = histogram;
    char *ws = (char *)workspace;
    a.hist = (unsigned long long *)ws;
    a.table = ws + hist_bytes(a.B, bins);
    a.inv_w = (double *)(ws + 2 * hist_bytes(a.B, bins));
    a.sums = (double *)(ws + 2 * hist_bytes(a.B, bins) + invw_bytes(a.B));
    a.st = (hipStream_t)stream;
    const int64_t count = (int64_t)a.B * bins * bins;
    const int64_t blocks = (count + ip::BLOCK - 1) / ip::BLOCK;
    hipLaunchKernelGGL((mi_clear<unsigned long long>), dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(ip::BLOCK), 0, a.st, a.hist, count);
    dispatch(p, a.k, [&](auto r, auto d, auto kmax) { mi_by_hessian<decltype(r), decltype(d)::value, decltype(kmax)::value>(a); });
    return hipGetLastError() == hipSuccess ? 0 : INTERPOL_E_LAUNCH;
}

} // extern "C"
