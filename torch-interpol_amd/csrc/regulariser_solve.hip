// ===========================================================================
// regulariser_solve.hip -- x = (H + L)^-1 g for displacement fields (B, *shape, D) by preconditioned conjugate gradients.
//
// L is the operator of regulariser.hip (reg_at, regulariser_at.hpp), H a symmetric positive semi-definite D x D matrix per
// lattice point (none, its diagonal, or diagonal + upper triangle row by row), M_o = H_o + diag(c) the preconditioner with
// c_d the interior diagonal of L, inverted per point in registers in closed form and never stored.
//
//     x = 0;  r = g;  z = M^-1 r;  p = z;  rho = <r,z>;  gamma = <g,g>;  done = (gamma == 0)
//     for k = 1 .. max_iter, items not done:
//         q = (H + L) p;   pi = <p,q>;   if pi <= 0 or rho <= 0: done, skip
//         alpha = rho/pi;  x += alpha p;  r -= alpha q;  z = M^-1 r;  rho' = <r,z>;  sigma = <r,r>;  iterations += 1
//         if sigma <= tolerance^2 gamma: done
//         beta = rho'/rho;  rho = rho';  p = z + beta p
//
//   solve_init<R, D, HK>       : x = 0, r = g, p = M^-1 g                        partial sums <r,z>, <g,g>
//   solve_matvec<R,D,MODE,HK>  : q = H p + L p (reg_at on p, H at the centre)    partial sum  <p,q>
//   solve_update<R, D, HK>     : x += alpha p, r -= alpha q, z = M^-1 r -> q     partial sums <r,z>, <r,r>
//   solve_direction<R>         : p = z + beta p
//   solve_scalars<PHASE>       : one workgroup per item after each reducing kernel: finishes the sums and writes alpha, beta,
//                                rho, the done flag, the iteration count and `info`
//
// Every iteration is enqueued from the one C call; alpha, beta and the stopping test stay on the device (no host
// synchronisation, no copy: safe under hipGraph capture).  The seams between the phases are kernel boundaries in stream order:
// no atomics, no grid-wide barrier, no spin wait, no cooperative launch; no workgroup reads a word that another workgroup of
// the same launch writes.  The reducing kernels are organised like reg_energy: RG_BLOCKS persistent workgroups per item over
// runs of consecutive points, one thread per point, every inner product a sum of DOUBLE products in a fixed order (the tree
// of an item depends neither on the shape nor on the batch: an item gives the same bits alone and inside a batch).  Every
// workgroup writes its slots, also when its run is empty or its item is done: the workspace is never assumed to be cleared.
// A done item is skipped by a branch that is uniform per workgroup; its x keeps its bits.
//
// HK (none / diagonal / full) is a template parameter everywhere: solve_matvec has 11 modes x 3 dims x 3 kinds x 2 types = 198
// instantiations.  With the elastic terms (interpol_regulariser_elastic_solve) c grows by
// h_d^2 [ shears sum_e 2 / h_e^2 + (shears + div) 2 / h_d^2 ]: the cross-component taps have none at the centre.  alpha and beta are doubles, rounded to R once where they
// multiply a field.
// The C entry points live here as well (include/interpol_hip.h: interpol_regulariser_solve).
// ===========================================================================
#include "regulariser_solve.hpp"

namespace ip {
namespace reg {

// slots (B, RG_BLOCKS, 2) doubles; scal (B, S_STRIDE) doubles; the fields x, r, p, q dense (B, N, D); g through p.vol_sb;
// H dense (N, K) per item with the batch stride hbs (0: one Hessian for every item)
template <typename R, int D, int HK>
__global__ __launch_bounds__(BLOCK) void solve_init(KParams p, Diag<R> c, const R *__restrict__ g, const R *__restrict__ H, int64_t hbs,
                                                    R *__restrict__ x, R *__restrict__ r, R *__restrict__ pp, double *__restrict__ slots, int B)
{
    typedef PointVec<R, D> V;
    constexpr int K = hess_count(D, HK);
    __shared__ double part[BLOCK / 64];
    int64_t lo, hi;
    run_of(p.N, blockIdx.x, lo, hi);
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        const R *gb = g + b * p.vol_sb, *hb = H + b * hbs;
        const int64_t fo = b * p.N * D;
        double acc0 = 0.0, acc1 = 0.0;
        for (int64_t o = lo + threadIdx.x; o < hi; o += BLOCK) {
            const V gv = *reinterpret_cast<const V *>(gb + o * D);
            R h[6];
            load_hess<R, K>(hb, o, h);
            V z, zero;
            precond<R, D, HK>(h, c, gv.c, z.c);
#pragma unroll
            for (int d = 0; d < D; ++d) {
                zero.c[d] = R(0);
                acc0 += (double)gv.c[d] * (double)z.c[d];
                acc1 += (double)gv.c[d] * (double)gv.c[d];
            }
            *reinterpret_cast<V *>(x + fo + o * D) = zero;
            *reinterpret_cast<V *>(r + fo + o * D) = gv;
            *reinterpret_cast<V *>(pp + fo + o * D) = z;
        }
        const double s0 = block_sum1(acc0, part), s1 = block_sum1(acc1, part);
        if (threadIdx.x == 0) {
            double *row = slots + (b * RG_BLOCKS + blockIdx.x) * 2;
            row[0] = s0;
            row[1] = s1;
        }
    }
}

template <typename R, int D, int MODE, int HK>
__global__ __launch_bounds__(BLOCK) void solve_matvec(KParams p, WeightsOf<R, MODE> w, const R *__restrict__ pp, const R *__restrict__ H,
                                                      int64_t hbs, R *__restrict__ q, double *__restrict__ slots,
                                                      const double *__restrict__ scal, int B)
{
    typedef PointVec<R, D> V;
    constexpr int K = hess_count(D, HK);
    __shared__ double part[BLOCK / 64];
    int64_t lo, hi;
    run_of(p.N, blockIdx.x, lo, hi);
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        double *row = slots + (b * RG_BLOCKS + blockIdx.x) * 2;
        if (scal[b * S_STRIDE + S_DONE] != 0.0) {                   // (uniform per item)
            if (threadIdx.x == 0) row[0] = 0.0;
            continue;
        }
        const int64_t fo = b * p.N * D;
        const V *ub = reinterpret_cast<const V *>(pp + fo);
        const R *hb = H + b * hbs;
        double acc = 0.0;
        for (int64_t o = lo + threadIdx.x; o < hi; o += BLOCK) {
            unsigned od[3];
            split_index<D>(p, o, od);
            V v0, lv;
            reg_at<R, D, MODE>(p, w, ub, od, v0, lv.c);
            R h[6];
            load_hess<R, K>(hb, o, h);
            hess_mul<R, D, HK>(h, v0.c, lv.c);
#pragma unroll
            for (int d = 0; d < D; ++d) acc += (double)v0.c[d] * (double)lv.c[d];
            *reinterpret_cast<V *>(q + fo + o * D) = lv;
        }
        const double s = block_sum1(acc, part);
        if (threadIdx.x == 0) row[0] = s;
    }
}

// z overwrites q in place: each thread reads q[o] before it writes z[o]
template <typename R, int D, int HK>
__global__ __launch_bounds__(BLOCK) void solve_update(KParams p, Diag<R> c, const R *__restrict__ H, int64_t hbs, R *__restrict__ x,
                                                      R *__restrict__ r, const R *__restrict__ pp, R *q, double *__restrict__ slots,
                                                      const double *__restrict__ scal, int B)
{
    typedef PointVec<R, D> V;
    constexpr int K = hess_count(D, HK);
    __shared__ double part[BLOCK / 64];
    int64_t lo, hi;
    run_of(p.N, blockIdx.x, lo, hi);
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        double *row = slots + (b * RG_BLOCKS + blockIdx.x) * 2;
        if (scal[b * S_STRIDE + S_DONE] != 0.0) {                   // (uniform per item)
            if (threadIdx.x == 0) { row[0] = 0.0; row[1] = 0.0; }
            continue;
        }
        const R alpha = (R)scal[b * S_STRIDE + S_ALPHA];
        const R *hb = H + b * hbs;
        const int64_t fo = b * p.N * D;
        double acc0 = 0.0, acc1 = 0.0;
        for (int64_t o = lo + threadIdx.x; o < hi; o += BLOCK) {
            const int64_t e = fo + o * D;
            V xv = *reinterpret_cast<const V *>(x + e), rv = *reinterpret_cast<const V *>(r + e);
            const V pv = *reinterpret_cast<const V *>(pp + e), qv = *reinterpret_cast<const V *>(q + e);
            R h[6];
            load_hess<R, K>(hb, o, h);
#pragma unroll
            for (int d = 0; d < D; ++d) {
                xv.c[d] = fma_(alpha, pv.c[d], xv.c[d]);
                rv.c[d] = fma_(-alpha, qv.c[d], rv.c[d]);
            }
            V z;
            precond<R, D, HK>(h, c, rv.c, z.c);
#pragma unroll
            for (int d = 0; d < D; ++d) {
                acc0 += (double)rv.c[d] * (double)z.c[d];
                acc1 += (double)rv.c[d] * (double)rv.c[d];
            }
            *reinterpret_cast<V *>(x + e) = xv;
            *reinterpret_cast<V *>(r + e) = rv;
            *reinterpret_cast<V *>(q + e) = z;
        }
        const double s0 = block_sum1(acc0, part), s1 = block_sum1(acc1, part);
        if (threadIdx.x == 0) { row[0] = s0; row[1] = s1; }
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------
// the workspace: r, p, q (B, N, D) each, the slots (B, RG_BLOCKS, 2) and the scalars (B, S_STRIDE); every part starts at a
// multiple of 256 bytes from the base
struct SolveLayout { int64_t r, p, q, slots, scal, total; };


static SolveLayout solve_layout(const KParams &k, int64_t B, int64_t es)
{
    const int64_t field = align256(B * k.N * k.dim * es);
    SolveLayout l;
    l.r = 0; l.p = field; l.q = 2 * field; l.slots = 3 * field;
    l.scal = l.slots + align256(B * RG_BLOCKS * 2 * (int64_t)sizeof(double));
    l.total = l.scal + align256(B * S_STRIDE * (int64_t)sizeof(double));
    return l;
}


struct SolveArgs {
    KParams k; WeightsEL<double> w; Diag<double> c; int mode, hk, B, max_iter; double tol2; int64_t hbs;
    const void *g, *H; void *x, *r, *p, *q; double *slots, *scal, *info; hipStream_t st;
};

template <typename R, int D, int HK>
static void solve_first(const SolveArgs &a, unsigned by)
{
    Diag<R> c;
    for (int d = 0; d < 3; ++d) c.c[d] = (R)a.c.c[d];
    hipLaunchKernelGGL((solve_init<R, D, HK>), dim3(RG_BLOCKS, by, 1), dim3(BLOCK), 0, a.st, a.k, c, (const R *)a.g, (const R *)a.H, a.hbs,
                       (R *)a.x, (R *)a.r, (R *)a.p, a.slots, a.B);
}

template <typename R, int D, int HK>
static void solve_step(const SolveArgs &a, unsigned by)
{
    Diag<R> c;
    for (int d = 0; d < 3; ++d) c.c[d] = (R)a.c.c[d];
    hipLaunchKernelGGL((solve_update<R, D, HK>), dim3(RG_BLOCKS, by, 1), dim3(BLOCK), 0, a.st, a.k, c, (const R *)a.H, a.hbs, (R *)a.x,
                       (R *)a.r, (const R *)a.p, (R *)a.q, a.slots, (const double *)a.scal, a.B);
}

template <typename R, int D, int MODE, int HK>
static void solve_apply_kind(const SolveArgs &a, unsigned by)
{
    hipLaunchKernelGGL((solve_matvec<R, D, MODE, HK>), dim3(RG_BLOCKS, by, 1), dim3(BLOCK), 0, a.st, a.k, WeightsOf<R, MODE>(narrow<R>(a.w)), (const R *)a.p,
                       (const R *)a.H, a.hbs, (R *)a.q, a.slots, (const double *)a.scal, a.B);
}

template <typename R, int D, int MODE>
static void solve_apply(const SolveArgs &a, unsigned by)
{
    switch (a.hk) {
    case HK_NONE: return solve_apply_kind<R, D, MODE, HK_NONE>(a, by);
    case HK_DIAG: return solve_apply_kind<R, D, MODE, HK_DIAG>(a, by);
    default: return solve_apply_kind<R, D, MODE, HK_FULL>(a, by);
    }
}

template <typename R, int D>
static void solve_apply_by_mode(const SolveArgs &a, unsigned by)
{
    switch (a.mode) {
    case 1: return solve_apply<R, D, 1>(a, by);
    case 2: return solve_apply<R, D, 2>(a, by);
    case 3: return solve_apply<R, D, 3>(a, by);
    case 4: return solve_apply<R, D, 4>(a, by);
    case 5: return solve_apply<R, D, 5>(a, by);
    case 6: return solve_apply<R, D, 6>(a, by);
    case 7: return solve_apply<R, D, 7>(a, by);
    case 10: return solve_apply<R, D, 10>(a, by);
    case 11: return solve_apply<R, D, 11>(a, by);
    case 14: return solve_apply<R, D, 14>(a, by);
    default: return solve_apply<R, D, 15>(a, by);
    }
}

template <typename R, int D>
static void solve_run(const SolveArgs &a)
{
    const unsigned by = (unsigned)(a.B < 65535 ? a.B : 65535);
    const int64_t n = a.k.N * D;
    const unsigned nb = (unsigned)((n + BLOCK - 1) / BLOCK);         // (< 2^24: N < 2^30)
    switch (a.hk) {
    case HK_NONE: solve_first<R, D, HK_NONE>(a, by); break;
    case HK_DIAG: solve_first<R, D, HK_DIAG>(a, by); break;
    default: solve_first<R, D, HK_FULL>(a, by); break;
    }
    hipLaunchKernelGGL((solve_scalars<0>), dim3(by), dim3(BLOCK), 0, a.st, (const double *)a.slots, a.scal, a.info, a.tol2, a.B);
    for (int it = 0; it < a.max_iter; ++it) {
        solve_apply_by_mode<R, D>(a, by);
        hipLaunchKernelGGL((solve_scalars<1>), dim3(by), dim3(BLOCK), 0, a.st, (const double *)a.slots, a.scal, a.info, a.tol2, a.B);
        switch (a.hk) {
        case HK_NONE: solve_step<R, D, HK_NONE>(a, by); break;
        case HK_DIAG: solve_step<R, D, HK_DIAG>(a, by); break;
        default: solve_step<R, D, HK_FULL>(a, by); break;
        }
        hipLaunchKernelGGL((solve_scalars<2>), dim3(by), dim3(BLOCK), 0, a.st, (const double *)a.slots, a.scal, a.info, a.tol2, a.B);
        if (it + 1 < a.max_iter)                                    // (the direction after the last update moves nothing in x)
            hipLaunchKernelGGL((solve_direction<R>), dim3(nb, by, 1), dim3(BLOCK), 0, a.st, n, (const R *)a.q, (R *)a.p, (const double *)a.scal, a.B);
    }
}

template <typename R>
static void solve_by_dim(const SolveArgs &a)
{
    switch (a.k.dim) {
    case 1: return solve_run<R, 1>(a);
    case 2: return solve_run<R, 2>(a);
    default: return solve_run<R, 3>(a);
    }
}


static int solve_entry(const interpol_problem *p, const void *gradient, const void *hessian, int hessian_components,
                       int64_t hessian_batch_stride, void *solution, const double *wt, bool sliding, const double *voxel_size,
                       int max_iter, double tolerance, void *info, void *workspace, int64_t workspace_bytes, void *stream)
{
    SolveArgs a;
    int slide = 0;
    int rc = solve_params(p, &a.k, &a.B, sliding ? &slide : nullptr);
    if (rc) return rc;
    if (!wt) return INTERPOL_E_NULL;
    a.mode = reg_weights(a.k.dim, wt[0], wt[1], wt[2], wt[3], wt[4], slide, voxel_size, &a.w);
    if (a.mode < 0) return a.mode;
    if (!reg_symmetric(a.k, slide, wt[3] > 0 || wt[4] > 0)) return INTERPOL_E_BOUND;
    a.hk = hess_kind(a.k.dim, hessian_components);
    if (a.hk < 0) return a.hk;
    if (max_iter < 0 || !(tolerance >= 0) || !(tolerance < 1e150)) return INTERPOL_E_SHAPE;
    if (hessian_batch_stride < 0) return INTERPOL_E_STRIDE;
    if (!gradient || !solution || !workspace || (a.hk != HK_NONE && !hessian)) return INTERPOL_E_NULL;
    const int D = a.k.dim;
    const int64_t B = a.B;
    const uint64_t es = p->dtype == INTERPOL_F64 ? 8 : 4;
    if ((uintptr_t)workspace % sizeof(double)) return INTERPOL_E_STRIDE;          // (the slots and the scalars are doubles)
    const SolveLayout l = solve_layout(a.k, B, (int64_t)es);
    if (workspace_bytes < l.total) return INTERPOL_E_SCRATCH;
    const uint64_t item = (uint64_t)a.k.N * D * es;
    const uint64_t gspan = (uint64_t)(B - 1) * (uint64_t)a.k.vol_sb * es + item;
    const uint64_t hitem = (uint64_t)a.k.N * hessian_components * es;
    const uint64_t hspan = a.hk == HK_NONE ? 0 : (uint64_t)(B - 1) * (uint64_t)hessian_batch_stride * es + hitem;
    const uint64_t xspan = (uint64_t)B * item, ispan = info ? (uint64_t)B * 2 * sizeof(double) : 0;
    // what is written (the solution, the workspace, info) overlaps neither an input nor each other
    const void *wr[3] = { solution, workspace, info };
    const uint64_t wn[3] = { xspan, (uint64_t)l.total, ispan };
    for (int i = 0; i < 3; ++i) {
        if (!wn[i]) continue;
        if (ranges_overlap(wr[i], wn[i], gradient, gspan) || (hspan && ranges_overlap(wr[i], wn[i], hessian, hspan))) return INTERPOL_E_STRIDE;
        for (int j = i + 1; j < 3; ++j)
            if (wn[j] && ranges_overlap(wr[i], wn[i], wr[j], wn[j])) return INTERPOL_E_STRIDE;
    }
    solve_centre(a.w, a.mode, D, &a.c);
    char *ws = (char *)workspace;
    a.g = gradient; a.H = hessian; a.hbs = a.hk == HK_NONE ? 0 : hessian_batch_stride;   // (no Hessian: never dereferenced)
    a.x = solution; a.r = ws + l.r; a.p = ws + l.p; a.q = ws + l.q;
    a.slots = (double *)(ws + l.slots); a.scal = (double *)(ws + l.scal); a.info = (double *)info;
    a.max_iter = max_iter; a.tol2 = tolerance * tolerance; a.st = (hipStream_t)stream;
    if (p->dtype == INTERPOL_F64) solve_by_dim<double>(a);
    else solve_by_dim<float>(a);
    return hipGetLastError() == hipSuccess ? 0 : INTERPOL_E_LAUNCH;
}

} // namespace reg
} // namespace ip

extern "C" {

int64_t interpol_regulariser_solve_workspace(const interpol_problem *p, int hessian_components)
{
    ip::KParams k; int B;
    const int rc = ip::reg::solve_params(p, &k, &B);
    if (rc) return rc;
    const int hk = ip::reg::hess_kind(k.dim, hessian_components);
    if (hk < 0) return hk;
    return ip::reg::solve_layout(k, B, p->dtype == INTERPOL_F64 ? 8 : 4).total;
}

int interpol_regulariser_solve(const interpol_problem *p, const void *gradient, const void *hessian, int hessian_components,
                               int64_t hessian_batch_stride, void *solution, double absolute, double membrane, double bending,
                               const double *voxel_size, int max_iter, double tolerance, void *info, void *workspace,
                               int64_t workspace_bytes, void *stream)
{
    const double wt[5] = { absolute, membrane, bending, 0.0, 0.0 };
    return ip::reg::solve_entry(p, gradient, hessian, hessian_components, hessian_batch_stride, solution, wt, false, voxel_size,
                                max_iter, tolerance, info, workspace, workspace_bytes, stream);
}

int64_t interpol_regulariser_elastic_solve_workspace(const interpol_problem *p, int hessian_components)
{
    ip::KParams k; int B, slide;
    const int rc = ip::reg::solve_params(p, &k, &B, &slide);
    if (rc) return rc;
    const int hk = ip::reg::hess_kind(k.dim, hessian_components);
    if (hk < 0) return hk;
    return ip::reg::solve_layout(k, B, p->dtype == INTERPOL_F64 ? 8 : 4).total;
}

int interpol_regulariser_elastic_solve(const interpol_problem *p, const void *gradient, const void *hessian, int hessian_components,
                                       int64_t hessian_batch_stride, void *solution, const double *weights, const double *voxel_size,
                                       int max_iter, double tolerance, void *info, void *workspace, int64_t workspace_bytes,
                                       void *stream)
{
    return ip::reg::solve_entry(p, gradient, hessian, hessian_components, hessian_batch_stride, solution, weights, true, voxel_size,
                                max_iter, tolerance, info, workspace, workspace_bytes, stream);
}

} // extern "C"
