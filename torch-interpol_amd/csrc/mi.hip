// ===========================================================================
// mi.hip -- the mutual-information data term of a Gauss-Newton step on a DENSE DISPLACEMENT FIELD: loss, gradient (B, *shape, D) and
// a per-voxel majoriser of the Hessian (B, *shape, K), one channel.  Four launches on one stream, one C call.
//
//     x(o) = o + disp[b, o, :],   I = mask(x) pull(moving, x),   G_d = mask(x) grad_d(moving, x),   J = fixed(o),   omega = weight mask
//     t_m, u, the taps, t_f, k, P, p_m, p_f, T, the loss, s, dI and c: those of mi_affine.hip
//     gradient[b, o, d] = dI G_d,   hessian[b, o, k] = c G_d G_e     k: the diagonal first, then the upper triangle row by row
//
//   mi_clear                     : (mi_common.hpp) clears the histogram region of the workspace.
//   mi_field_histogram<R, D, KMAX> : MI_BLOCKS persistent workgroups per item, which loop over the boxes of point_field.hpp (3-D:
//       4 x 2 x 32 samples, so that the stencils of a wave under a rough field overlap in two dims; D < 3: 256 samples in storage
//       order).  Per sample the displacement branch of load_coords in R and ONE Stencil, evaluated in DOUBLE from the tensors'
//       values together with u, k and beta3 (mi_affine.hip, sample_value_double, says why); four fixed-point updates (ds_add_u64)
//       into a B x B histogram of 64-bit integers in LDS; the non-zero bins go to the item's histogram in the workspace with 64-bit
//       integer atomics.  The quantum is that of mi_affine.hip.  Integer sums are exact in any order: the histogram does not
//       depend on the run, on the number of workgroups, on the map from workgroups to samples or on the batch the item sits in.
//   mi_table<R>                  : (mi_common.hpp) one workgroup per item: P, p_m, p_f, T and the loss in double; T rounded once to R
//       and 1 / W into the workspace.  A total <= 0 (W = 0) gives T = 0, 1 / W = 0, loss = 0: every output is zero.
//   mi_field_terms<R, D, KMAX, HK> : one thread per sample (compose_sample), T staged in LDS; ONE Stencil<R, D, KMAX, true, NEED_G>
//       for the value and the D derivative sums, sample_bins, dI and c as mi_affine.hip's MiTerms forms them, one PointVec<R, D>
//       and one PointVec<R, K> store.  Threads past the lattice store nothing; out-of-view samples store zeros (omega = 0, G = 0).
//       No sums, no slots, no atomics: the stencil is recomputed, nothing but the two fields is written.
//
// No floating-point atomics: two calls give identical bits, an item gives the same bits alone or inside a batch, and the launches
// replay from a captured graph to the bits of eager.  Instantiated for float / double, D = 1..3, one order 1..3, HK = 0..2,
// 8 <= B <= 64 (a run-time value: the LDS of the histogram and of T is sized at launch).  The C entry points live here as well
// (include/interpol_hip.h: interpol_mi_workspace, interpol_mi).  data_term.hpp holds the validation of the problem, the alias
// check, the Hessian layouts, the stencil loops and the dispatch; mi_common.hpp what the two mutual-information terms share.
// ===========================================================================
#include "mi_common.hpp"
#include "point_field.hpp"                                         // PointVec, compose_sample, compose_blocks

namespace ip {
namespace mi_dense {

using namespace ip::mi;

// the batch strides (elements) the problem descriptor has no field for
struct Strides { int64_t weight, gradient, hessian; };

// ---- stage 1: the joint histogram in 64-bit fixed point ----------------------------------------------------------------
// hist (B, bins, bins) of 64-bit integers, cleared by mi_clear before the launch; ranges (B, RANGE_STRIDE) doubles; nboxes:
// compose_blocks of the lattice
template <typename R, int D, int KMAX>
__global__ __launch_bounds__(BLOCK) void mi_field_histogram(KParams p, const R *__restrict__ moving, const R *__restrict__ fixed,
                                                            const R *__restrict__ disp, const R *__restrict__ weight,
                                                            const double *__restrict__ ranges, unsigned long long *__restrict__ hist,
                                                            int64_t weight_sb, unsigned nboxes, int bins, int shift)
{
    extern __shared__ unsigned long long lh[];                      // bins x bins
    const int64_t b = blockIdx.y;
    const R *mb = moving + b * p.vol_sb;
    const R *fb = fixed + b * p.val_sb;
    const R *wb = weight ? weight + b * weight_sb : nullptr;
    const double *rg = ranges + b * RANGE_STRIDE;
    const double m_lo = rg[0], m_sc = rg[1], f_lo = rg[2], f_sc = rg[3];
    const double wmax = rg[4];
    const double inv_q = wmax > 0.0 ? ldexp(1.0, shift) / wmax : 0.0;
    const int nb = bins * bins;
    for (int i = threadIdx.x; i < nb; i += BLOCK) lh[i] = 0ull;
    __syncthreads();
    for (unsigned bi = blockIdx.x; bi < nboxes; bi += MI_BLOCKS) {
#ifdef IP_MI_HISTOGRAM_ROWS                                         // (the samples in storage order in 3-D as well: the A/B of profiles/mi.txt)
        const int64_t o = compose_sample<D == 3 ? 2 : D>(p, bi);
#else
        const int64_t o = compose_sample<D>(p, bi);
#endif
        if (o < 0) continue;                                        // (a thread past the lattice in a partial box)
        double x[D];
        load_coords<double, R, D>(p, disp, b, o, x);
        Stencil<double, D, KMAX, true, NEED_W> s;
        s.setup(p, x);
        const double wt = wb ? (double)wb[o] : 1.0;
        opaque(s);
        double aw = 0.0;
        IP_STENCIL_VALUE(s, mb, aw);
        const double I = aw * s.mask, omega = wt * s.mask;
        const Bins<double> sb = sample_bins<double>(I, (double)fb[o], m_lo, m_sc, f_lo, f_sc, bins);
        double w[4];
        bspline3<double>(sb.f, w);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long long v = __double2ll_rn((omega * w[i]) * inv_q);
            if (v) atomicAdd(&lh[(sb.j0 + i) * bins + sb.k], (unsigned long long)v);     // ds_add_u64; 0 <= j0 + i < bins, 0 <= k < bins
        }
    }
    __syncthreads();
    unsigned long long *hb = hist + b * nb;
    for (int i = threadIdx.x; i < nb; i += BLOCK) {
        const unsigned long long v = lh[i];
        if (v) __hip_atomic_fetch_add(hb + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- stage 3: the two fields ------------------------------------------------------------------------------------------------
// table (B, bins, bins) of R and inv_w (B) doubles from mi_table; gradient (B, *shape, D), hessian (B, *shape, K) through sb
template <typename R, int D, int KMAX, int HK>
__global__ __launch_bounds__(BLOCK) void mi_field_terms(KParams p, const R *__restrict__ moving, const R *__restrict__ fixed,
                                                        const R *__restrict__ disp, const R *__restrict__ weight,
                                                        const double *__restrict__ ranges, const R *__restrict__ table,
                                                        const double *__restrict__ inv_w, R *__restrict__ gradient,
                                                        R *__restrict__ hessian, Strides sb, int bins)
{
    constexpr int K = HK == HK_NONE ? 1 : hess_components(D, HK);
    constexpr bool HESS = HK != HK_NONE;
    typedef PointVec<R, D> V;
    typedef PointVec<R, K> H;
    const int64_t b = blockIdx.y;
    const R *T = stage_table<R>(table, b, bins);                    // (every thread of the workgroup: it synchronises)
    const int64_t o = compose_sample<D>(p);
    if (o < 0) return;                                              // a thread past the lattice
    const double *rg = ranges + b * RANGE_STRIDE;
    const R m_lo = (R)rg[0], m_sc = (R)rg[1], f_lo = (R)rg[2], f_sc = (R)rg[3], iw = (R)inv_w[b];
    R x[D];
    load_coords<R, R, D>(p, disp, b, o, x);
    Stencil<R, D, KMAX, true, NEED_G> s;
    s.setup(p, x);
    const R wt = weight ? weight[b * sb.weight + o] : R(1);
    const R *v0 = moving + b * p.vol_sb;
    opaque(s);
    R a0 = R(0), a1 = R(0), a2 = R(0), aw = R(0);
    IP_STENCIL_VALUE_GRADIENT(s, v0, aw, a0, a1, a2);
    const R acc[3] = { a0, a1, a2 };
    R G[D];
#pragma unroll
    for (int d = 0; d < D; ++d) G[d] = acc[d] * s.mask;
    const R I = aw * s.mask, omega = wt * s.mask;
    const Bins<R> sn = sample_bins<R>(I, fixed[b * p.val_sb + o], m_lo, m_sc, f_lo, f_sc, bins);
    R d1[4], d2[4];
    bspline3_d1<R>(sn.f, d1);
    if (HESS) bspline3_abs_d2<R>(sn.f, d2);
    R a = R(0), c = R(0);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const R t = T[(sn.j0 + i) * bins + sn.k];                   // 0 <= j0 + i < bins, 0 <= k < bins (sample_bins)
        a = fma_(d1[i], t, a);
        if (HESS) c = fma_(d2[i], fabs(t), c);
    }
    const R sc = sn.clamped ? R(0) : (R)(bins - 4) * m_sc;
    const R wn = omega * iw;
    const R dI = -(wn * sc) * a;
    V gv;
#pragma unroll
    for (int d = 0; d < D; ++d) gv.c[d] = dI * G[d];
    *reinterpret_cast<V *>(gradient + b * sb.gradient + o * D) = gv;
    if (HESS) {
        const R cc = (wn * sc) * sc * c;
        H hv;
#pragma unroll
        for (int d = 0; d < D; ++d) hv.c[d] = cc * G[d] * G[d];
        if (HK == HK_FULL) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
#pragma unroll
                for (int e = d + 1; e < D; ++e) hv.c[diag_first_index(d, e, D)] = cc * G[d] * G[e];
            }
        }
        *reinterpret_cast<H *>(hessian + b * sb.hessian + o * K) = hv;
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------
// workgroups of mi_field_terms per batch item = boxes of mi_field_histogram: a function of the sample lattice alone
static int64_t mi_boxes(const KParams &k)
{
    switch (k.dim) {
    case 1: return compose_blocks<1>(k);
    case 2: return compose_blocks<2>(k);
    default: return compose_blocks<3>(k);
    }
}

struct Args {
    KParams k; int B; int hk; int64_t nb; int bins, shift; Strides sb;
    const void *moving, *fixed, *disp, *weight; const double *ranges; void *loss, *gradient, *hessian, *histogram;
    unsigned long long *hist; void *table; double *inv_w; hipStream_t st;
};

// the workspace: the integer histograms, T (8 bytes per entry reserved), 1 / W
static int64_t mi_workspace(int B, int bins) { return 2 * hist_bytes(B, bins) + invw_bytes(B); }

template <typename R, int D, int KMAX, int HK>
static void mi_launch(const Args &a)
{
    const unsigned nbin = (unsigned)(a.bins * a.bins);
    hipLaunchKernelGGL((mi_field_histogram<R, D, KMAX>), dim3(MI_BLOCKS, (unsigned)a.B, 1), dim3(BLOCK), nbin * 8, a.st, a.k,
                       (const R *)a.moving, (const R *)a.fixed, (const R *)a.disp, (const R *)a.weight, a.ranges, a.hist, a.sb.weight,
                       (unsigned)a.nb, a.bins, a.shift);
    hipLaunchKernelGGL((mi_table<R>), dim3((unsigned)a.B), dim3(BLOCK), 0, a.st, (const long long *)a.hist, a.ranges, (R *)a.table,
                       a.inv_w, (R *)a.loss, (R *)a.histogram, a.bins, a.shift);
    hipLaunchKernelGGL((mi_field_terms<R, D, KMAX, HK>), dim3((unsigned)a.nb, (unsigned)a.B, 1), dim3(BLOCK), nbin * sizeof(R), a.st, a.k,
                       (const R *)a.moving, (const R *)a.fixed, (const R *)a.disp, (const R *)a.weight, a.ranges, (const R *)a.table,
                       (const double *)a.inv_w, (R *)a.gradient, (R *)a.hessian, a.sb, a.bins);
}

template <typename R, int D, int KMAX>
static void mi_by_hessian(const Args &a)
{
    switch (a.hk) {
    case HK_NONE: return mi_launch<R, D, KMAX, HK_NONE>(a);
    case HK_DIAG: return mi_launch<R, D, KMAX, HK_DIAG>(a);
    default: return mi_launch<R, D, KMAX, HK_FULL>(a);
    }
}

// the problem of interpol_ssd with one channel, the bins, and a batch that fits gridDim.y
static int mi_params(const interpol_problem *p, int bins, KParams *k, int *B, uint64_t *mspan, int64_t *nb)
{
    const int rc = problem_params(p, LATTICE_FIELD, k, B, mspan);
    if (rc) return rc;
    if (k->C != 1) return INTERPOL_E_SHAPE;
    if (bins < MIN_BINS || bins > MAX_BINS) return INTERPOL_E_SHAPE;
    if (*B > 65535) return INTERPOL_E_SHAPE;                        // the item sits on gridDim.y
    *nb = mi_boxes(*k);
    if (*nb > 0x7fffffffll) return INTERPOL_E_SHAPE;                // (a thin 3-D lattice of more than 2^31 boxes)
    return 0;
}

} // namespace mi_dense
} // namespace ip

extern "C" {

int64_t interpol_mi_workspace(const interpol_problem *p, int bins)
{
    ip::KParams k; int B; uint64_t mspan; int64_t nb;
    const int rc = ip::mi_dense::mi_params(p, bins, &k, &B, &mspan, &nb);
    if (rc) return rc;
    return ip::mi_dense::mi_workspace(B, bins);
}

int interpol_mi(const interpol_problem *p, const void *moving, const void *fixed, const void *disp, const void *weight,
                const void *ranges, void *loss, void *gradient, void *hessian, void *histogram, int hessian_kind, int bins,
                int64_t weight_batch_stride, int64_t gradient_batch_stride, int64_t hessian_batch_stride, void *workspace,
                int64_t workspace_bytes, void *stream)
{
    using namespace ip::mi_dense;
    Args a;
    uint64_t mimage;
    const int rc = mi_params(p, bins, &a.k, &a.B, &mimage, &a.nb);
    if (rc) return rc;
    if (hessian_kind != HK_NONE && hessian_kind != HK_DIAG && hessian_kind != HK_FULL) return INTERPOL_E_SHAPE;
    a.hk = hessian_kind;
    a.bins = bins;
    const int D = a.k.dim, K = hess_components(D, a.hk);
    const uint64_t B = (uint64_t)a.B, N = (uint64_t)a.k.N, NB = (uint64_t)bins * (uint64_t)bins;
    const uint64_t es = p->dtype == INTERPOL_F64 ? 8 : 4;
    if (gradient_batch_stride < 0 || (weight && weight_batch_stride < 0) || (K && hessian_batch_stride < 0)) return INTERPOL_E_STRIDE;
    // the outputs have an item of their own per batch item
    if (B > 1 && ((uint64_t)gradient_batch_stride < N * D || (K && (uint64_t)hessian_batch_stride < N * K))) return INTERPOL_E_STRIDE;
    if (!moving || !fixed || !disp || !ranges || !loss || !gradient || !workspace || (K && !hessian)) return INTERPOL_E_NULL;
    if ((uintptr_t)workspace % sizeof(double) || (uintptr_t)ranges % sizeof(double)) return INTERPOL_E_STRIDE;   // (doubles)
    const uint64_t wsbytes = (uint64_t)mi_workspace(a.B, bins);
    if (workspace_bytes < (int64_t)wsbytes) return INTERPOL_E_SCRATCH;
    // what is written (loss, gradient, hessian, histogram, workspace) overlaps neither an input nor each other
    const Range rd[5] = { { moving, moving_bytes(a.k, B, es, mimage) }, { fixed, fixed_bytes(a.k, B, es) },
                          { disp, ((B - 1) * (uint64_t)a.k.grid_sb + N * D) * es }, { weight, weight_bytes(a.k, B, es, weight, weight_batch_stride) },
                          { ranges, B * RANGE_STRIDE * sizeof(double) } };
    const Range wr[5] = { { loss, B * es }, { gradient, ((B - 1) * (uint64_t)gradient_batch_stride + N * D) * es },
                          { hessian, K ? ((B - 1) * (uint64_t)hessian_batch_stride + N * K) * es : 0 },
                          { histogram, histogram ? B * NB * es : 0 }, { workspace, wsbytes } };
    if (ranges_alias(rd, 5, wr, 5)) return INTERPOL_E_STRIDE;
    a.shift = quantum_shift(a.k.N);
    a.sb.weight = weight ? weight_batch_stride : 0;
    a.sb.gradient = gradient_batch_stride;
    a.sb.hessian = K ? hessian_batch_stride : 0;                    // (no Hessian: never dereferenced)
    a.moving = moving; a.fixed = fixed; a.disp = disp; a.weight = weight; a.ranges = (const double *)ranges;
    a.loss = loss; a.gradient = gradient; a.hessian = K ? hessian : nullptr; a.histogram = histogram;
    char *ws = (char *)workspace;
    a.hist = (unsigned long long *)ws;
    a.table = ws + hist_bytes(a.B, bins);
    a.inv_w = (double *)(ws + 2 * hist_bytes(a.B, bins));
    a.st = (hipStream_t)stream;
    const int64_t count = (int64_t)a.B * bins * bins;
    const int64_t blocks = (count + ip::BLOCK - 1) / ip::BLOCK;
    hipLaunchKernelGGL((mi_clear<unsigned long long>), dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(ip::BLOCK), 0, a.st, a.hist, count);
    dispatch(p, a.k, [&](auto r, auto d, auto kmax) { mi_by_hessian<decltype(r), decltype(d)::value, decltype(kmax)::value>(a); });
    return hipGetLastError() == hipSuccess ? 0 : INTERPOL_E_LAUNCH;
}

} // extern "C"
