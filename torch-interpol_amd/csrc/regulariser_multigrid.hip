// ===========================================================================
// regulariser_multigrid.hip -- the conjugate gradients of regulariser_solve.hip with a multigrid V-cycle as preconditioner:
// z = V(r) in the place of z = M^-1 r, in the initialisation and in the loop; rho, pi, alpha, beta, sigma, the guards, the
// stopping test and `info` are those of regulariser_solve.hip (solve_scalars and solve_direction are shared).
//
// Levels.  Level 0 is the call's lattice.  Dimension d is halved from one level to the next iff n_d is even and n_d / 2 >= 4
// (semi-coarsening: an odd dft dimension cannot be halved without breaking the period); the last level is the one on which
// no dimension can be halved.  s_d = 2 where d was halved, else 1; h_{l+1,d} = s_d h_{l,d}; kappa_{l+1} = kappa_l prod_d s_d.
//   A_l = H_l + L(kappa_l weights, h_l, bound)        (reg_at with the tables of the level: a coarse voxel stands for kappa fine ones)
//   M_l = H_l + diag(c(kappa_l weights, h_l))         (inverted per point in closed form: precond of regulariser_solve.hpp)
//   P_l : cell-centred linear interpolation along each halved dimension, fine i = 3/4 e[i >> 1] + 1/4 e[(i >> 1) -+ 1] (minus
//         for even i), an out-of-range coarse index extended by the bound of that dimension FOR THAT COMPONENT (sliding: dst2
//         for c = d, dct2 otherwise), the identity along the others; component c times s_c (coarse voxels -> fine voxels)
//   R_l = P_l^T as a gather: coarse j sums fine 2j-1, 2j, 2j+1, 2j+2 with 1/4, 3/4, 3/4, 1/4, the same extension on the fine field
//   H_{l+1}[o] = S (sum over the prod s_d children of o of H_l) S,  S = diag(s): entry (c, e) times s_c s_e
//
//   V(l, r):  x = 0;  nu sweeps x <- x + omega M_l^-1 (r - A_l x)   (omega = 1/2; nu = smoothing, 8 on the last level, which
//             returns x; the first sweep is omega M^-1 r);  d = r - A_l x;  x <- x + P_l V(l + 1, P_l^T d);  nu more sweeps
//
//   mg_first<R,D,HK>            : x = omega M^-1 r
//   mg_apply<R,D,MODE,HK>       : op 0: out = A x (the matvec of the conjugate gradients); 1: out = r - A x; 2: out = x + omega M^-1 (r - A x)
//   mg_restrict<R,D,MASK>       : r_{l+1} = P^T d   (MASK: the halved dimensions; at most 4^D loads per coarse point)
//   mg_prolong_add<R,D,MASK>    : x_l += P e        (at most 2^D loads per fine point, in place: a thread touches its own point only)
//   mg_coarsen_hess<R,D,K,MASK> : H_{l+1} from H_l, once per call
//   mgcg_init, mgcg_dot, mgcg_update : the element-wise passes of the conjugate gradients with their fixed-order sums
//
// Every kernel is a gather with one thread per lattice point (experiments/regulariser_tile.inc: the LDS halo tile measured
// slower for this stencil), loops over the batch, and writes no word that another thread reads in the same launch: no
// atomics, no grid-wide barrier, bit-identical from run to run and for an item alone or inside a batch.  The whole cycle is
// enqueued from the one C call inside the loop of the conjugate gradients: no host synchronisation, safe under hipGraph
// capture.  The first cycle (before the scalars exist) runs for every item; later ones skip an item that is done by a branch
// that is uniform per item, like every other pass: its x, r and p keep their bits, and what the skipped cycle leaves in z is
// never read (solve_scalars and solve_direction skip the item too).
// Sweeps ping-pong between two buffers a and b per level; d = r - A x goes to the idle one of the two.  After 2 nu sweeps (or
// 8 on the last level) the result is always in b.
// ===========================================================================
#include "regulariser_solve.hpp"

namespace ip {
namespace reg {

constexpr int MG_MAX_LEVELS = 32;                                   // (N < 2^30: at most 30 halvings)
constexpr int MG_COARSEST_SWEEPS = 8;

template <typename R> struct Scale { R s[3]; };

// ---- the level operator ---------------------------------------------------------------------------------------------------
// r through the batch stride rsb (elements), x and out dense (B, N, D)
template <typename R, int D, int HK>
__global__ __launch_bounds__(BLOCK) void mg_first(int64_t N, Diag<R> c, const R *__restrict__ r, int64_t rsb, const R *__restrict__ H,
                                                  int64_t hbs, R *__restrict__ out, const double *__restrict__ scal, int B)
{
    typedef PointVec<R, D> V;
    constexpr int K = hess_count(D, HK);
    const int64_t o = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (o >= N) return;
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        if (scal && scal[b * S_STRIDE + S_DONE] != 0.0) continue;       // (uniform per item: a finished item is not cycled)
        const V rv = *reinterpret_cast<const V *>(r + b * rsb + o * D);
        R h[6];
        load_hess<R, K>(H + b * hbs, o, h);
        V z;
        precond<R, D, HK>(h, c, rv.c, z.c);
#pragma unroll
        for (int d = 0; d < D; ++d) z.c[d] = R(0.5) * z.c[d];
        *reinterpret_cast<V *>(out + (b * N + o) * D) = z;
    }
}

template <typename R, int D, int MODE, int HK>
__global__ __launch_bounds__(BLOCK) void mg_apply(KParams p, WeightsOf<R, MODE> w, Diag<R> c, int op, const R *__restrict__ x,
                                                  const R *__restrict__ r, int64_t rsb, const R *__restrict__ H, int64_t hbs,
                                                  R *__restrict__ out, const double *__restrict__ scal, int B)
{
    typedef PointVec<R, D> V;
    constexpr int K = hess_count(D, HK);
    const int64_t o = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (o >= p.N) return;
    unsigned od[3];
    split_index<D>(p, o, od);
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        if (scal && scal[b * S_STRIDE + S_DONE] != 0.0) continue;       // (uniform per item: a finished item is not cycled)
        const int64_t fo = b * p.N * D;
        V v0, lv;
        reg_at<R, D, MODE>(p, w, reinterpret_cast<const V *>(x + fo), od, v0, lv.c);
        R h[6];
        load_hess<R, K>(H + b * hbs, o, h);
        hess_mul<R, D, HK>(h, v0.c, lv.c);
        if (op != 0) {                                              // (uniform)
            const V rv = *reinterpret_cast<const V *>(r + b * rsb + o * D);
#pragma unroll
            for (int d = 0; d < D; ++d) lv.c[d] = rv.c[d] - lv.c[d];
            if (op == 2) {
                V z;
                precond<R, D, HK>(h, c, lv.c, z.c);
#pragma unroll
                for (int d = 0; d < D; ++d) lv.c[d] = fma_(R(0.5), z.c[d], v0.c[d]);
            }
        }
        *reinterpret_cast<V *>(out + fo + o * D) = lv;
    }
}

// ---- grid transfer ------------------------------------------------------------------------------------------------------
// index and signs of tap i along a dimension of extent n: sg for every component, so for the component of that dimension
// (they differ in a sliding dimension alone); the index is always inside [0, n)
__device__ __forceinline__ void mg_tap(int bd, bool sliding, int i, int n, int &idx, int &sg, int &so)
{
    idx = i; sg = 1; so = 1;
    if ((unsigned)i >= (unsigned)n) {
        const long long pk = wrap_outofline(bd, i, n);
        idx = (int)(pk & 0xffffffffll);
        sg = so = (int)(pk >> 32);
        if (sliding) so = (int)(wrap_outofline(B_DST2, i, n) >> 32);
    }
}

// fine (B, Nf, D) -> coarse (B, Nc, D); pc: the coarse level (gshape), nf: the fine extents.  The taps of dimensions 1 and 2 are
// held (16 loads in flight); those of dimension 0 are formed one after the other in a loop that is not unrolled (all 64 taps of the
// 3-D kernel with their three weights unrolled need more than 256 VGPRs).
template <typename R, int D, int MASK>
__global__ __launch_bounds__(BLOCK) void mg_restrict(KParams pc, int nf0, int nf1, int nf2, int slide, Scale<R> sc, int64_t Nf,
                                                     const R *__restrict__ fine, R *__restrict__ coarse, const double *__restrict__ scal, int B)
{
    typedef PointVec<R, D> V;
    constexpr int NT0 = (MASK & 1) ? 4 : 1, NT1 = (MASK & 2) ? 4 : 1, NT2 = (MASK & 4) ? 4 : 1;
    const int64_t o = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (o >= pc.N) return;
    unsigned od[3] = { 0, 0, 0 };
    split_index<D>(pc, o, od);
    const int nf[3] = { nf0, nf1, nf2 };
    unsigned off[3][4];
    R w[3][4], wo[3][4];
    unsigned fs = 1;                                                // the stride of dimension d of the fine field, in points
#pragma unroll
    for (int d = 2; d >= 1; --d) {
#pragma unroll
        for (int t = 0; t < 4; ++t) { off[d][t] = 0; w[d][t] = R(1); wo[d][t] = R(1); }
        if (d >= D) continue;
        if ((MASK >> d) & 1) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                int idx, sg, so;
                mg_tap(pc.bound[d], (slide >> d) & 1, 2 * (int)od[d] - 1 + t, nf[d], idx, sg, so);
                const R q = (t == 0 || t == 3) ? R(0.25) : R(0.75);
                off[d][t] = (unsigned)idx * fs;
                w[d][t] = q * R(sg);
                wo[d][t] = q * R(so);
            }
        } else {
            off[d][0] = od[d] * fs;
        }
        fs *= (unsigned)nf[d];
    }
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        if (scal && scal[b * S_STRIDE + S_DONE] != 0.0) continue;       // (uniform per item: a finished item is not cycled)
        const V *fb = reinterpret_cast<const V *>(fine + b * Nf * D);
        R acc[D];
#pragma unroll
        for (int c = 0; c < D; ++c) acc[c] = R(0);
#pragma unroll 1
        for (int t0 = 0; t0 < NT0; ++t0) {
            unsigned off0 = od[0] * fs;
            R w0 = R(1), wo0 = R(1);
            if (MASK & 1) {
                int idx, sg, so;
                mg_tap(pc.bound[0], slide & 1, 2 * (int)od[0] - 1 + t0, nf0, idx, sg, so);
                const R q = (t0 == 0 || t0 == 3) ? R(0.25) : R(0.75);
                off0 = (unsigned)idx * fs;
                w0 = q * R(sg);
                wo0 = q * R(so);
            }
#pragma unroll
            for (int t1 = 0; t1 < NT1; ++t1) {
#pragma unroll
                for (int t2 = 0; t2 < NT2; ++t2) {
                    const V v = fb[off0 + off[1][t1] + off[2][t2]];
                    acc[0] = fma_(wo0 * (w[1][t1] * w[2][t2]), v.c[0], acc[0]);
                    if constexpr (D > 1) acc[1] = fma_(w0 * (wo[1][t1] * w[2][t2]), v.c[1], acc[1]);
                    if constexpr (D > 2) acc[2] = fma_(w0 * (w[1][t1] * wo[2][t2]), v.c[2], acc[2]);
                }
            }
        }
        V out;
#pragma unroll
        for (int c = 0; c < D; ++c) out.c[c] = sc.s[c] * acc[c];
        *reinterpret_cast<V *>(coarse + (b * pc.N + o) * D) = out;
    }
}

// x_fine += P coarse; pf: the fine level (gshape), nc: the coarse extents
template <typename R, int D, int MASK>
__global__ __launch_bounds__(BLOCK) void mg_prolong_add(KParams pf, int nc0, int nc1, int nc2, int slide, Scale<R> sc, int64_t Nc,
                                                        const R *__restrict__ coarse, R *__restrict__ fine, const double *__restrict__ scal, int B)
{
    typedef PointVec<R, D> V;
    constexpr int NT0 = (MASK & 1) ? 2 : 1, NT1 = (MASK & 2) ? 2 : 1, NT2 = (MASK & 4) ? 2 : 1;
    const int64_t o = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (o >= pf.N) return;
    unsigned od[3] = { 0, 0, 0 };
    split_index<D>(pf, o, od);
    const int nc[3] = { nc0, nc1, nc2 };
    unsigned off[3][2];
    R w[3][2], wo[3][2];
    unsigned cs = 1;
#pragma unroll
    for (int d = 2; d >= 0; --d) {
#pragma unroll
        for (int t = 0; t < 2; ++t) { off[d][t] = 0; w[d][t] = R(1); wo[d][t] = R(1); }
        if (d >= D) continue;
        if ((MASK >> d) & 1) {
            const int j = (int)(od[d] >> 1);
            int idx, sg, so;
            mg_tap(pf.bound[d], (slide >> d) & 1, (od[d] & 1) ? j + 1 : j - 1, nc[d], idx, sg, so);
            off[d][0] = (unsigned)j * cs;   w[d][0] = R(0.75);          wo[d][0] = R(0.75);
            off[d][1] = (unsigned)idx * cs; w[d][1] = R(0.25) * R(sg);  wo[d][1] = R(0.25) * R(so);
        } else {
            off[d][0] = od[d] * cs;
        }
        cs *= (unsigned)nc[d];
    }
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        if (scal && scal[b * S_STRIDE + S_DONE] != 0.0) continue;       // (uniform per item: a finished item is not cycled)
        const V *cb = reinterpret_cast<const V *>(coarse + b * Nc * D);
        R acc[D];
#pragma unroll
        for (int c = 0; c < D; ++c) acc[c] = R(0);
#pragma unroll
        for (int t0 = 0; t0 < NT0; ++t0) {
#pragma unroll
            for (int t1 = 0; t1 < NT1; ++t1) {
#pragma unroll
                for (int t2 = 0; t2 < NT2; ++t2) {
                    const V v = cb[off[0][t0] + off[1][t1] + off[2][t2]];
                    const int t[3] = { t0, t1, t2 };
#pragma unroll
                    for (int c = 0; c < D; ++c) {
                        R q = R(1);
#pragma unroll
                        for (int d = 0; d < D; ++d) q *= d == c ? wo[d][t[d]] : w[d][t[d]];
                        acc[c] = fma_(q, v.c[c], acc[c]);
                    }
                }
            }
        }
        V *xp = reinterpret_cast<V *>(fine + (b * pf.N + o) * D);
        V xv = *xp;
#pragma unroll
        for (int c = 0; c < D; ++c) xv.c[c] = fma_(sc.s[c], acc[c], xv.c[c]);
        *xp = xv;
    }
}

// H_{l+1}[o] = S (sum of the children) S; Hf (Nf, K) per item with the batch stride hbs (0: one for all, then Bh = 1), Hc dense
// (Bh, Nc, K).  se: s_c s_e of the K packed entries
template <typename R> struct Scale6 { R s[6]; };

template <typename R, int D, int K, int MASK>
__global__ __launch_bounds__(BLOCK) void mg_coarsen_hess(KParams pc, int nf0, int nf1, int nf2, Scale6<R> se, const R *__restrict__ Hf,
                                                         int64_t hbs, R *__restrict__ Hc, int Bh)
{
    typedef PointVec<R, K> V;
    constexpr int NT0 = (MASK & 1) ? 2 : 1, NT1 = (MASK & 2) ? 2 : 1, NT2 = (MASK & 4) ? 2 : 1;
    const int64_t o = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (o >= pc.N) return;
    unsigned od[3] = { 0, 0, 0 };
    split_index<D>(pc, o, od);
    const int nf[3] = { nf0, nf1, nf2 };
    unsigned st[3] = { 0, 0, 0 }, base = 0, fs = 1;                 // the strides of the fine lattice, in points
#pragma unroll
    for (int d = D - 1; d >= 0; --d) {
        st[d] = fs;
        base += (((MASK >> d) & 1) ? 2 * od[d] : od[d]) * fs;
        fs *= (unsigned)nf[d];
    }
    for (int64_t b = blockIdx.y; b < Bh; b += gridDim.y) {
        const V *hb = reinterpret_cast<const V *>(Hf + b * hbs);
        R acc[K];
#pragma unroll
        for (int i = 0; i < K; ++i) acc[i] = R(0);
#pragma unroll
        for (int t0 = 0; t0 < NT0; ++t0) {
#pragma unroll
            for (int t1 = 0; t1 < NT1; ++t1) {
#pragma unroll
                for (int t2 = 0; t2 < NT2; ++t2) {
                    const V v = hb[base + t0 * st[0] + t1 * st[1] + t2 * st[2]];
#pragma unroll
                    for (int i = 0; i < K; ++i) acc[i] += v.c[i];
                }
            }
        }
        V out;
#pragma unroll
        for (int i = 0; i < K; ++i) out.c[i] = se.s[i] * acc[i];
        *reinterpret_cast<V *>(Hc + (b * pc.N + o) * K) = out;
    }
}

// ---- the element-wise passes of the conjugate gradients ---------------------------------------------------------------
// The reducing kernels: workgroup g of nb sums the run g of the n = N D elements of an item (run_of; nb = the runs that are
// not empty); workgroup 0 also writes the zeros of the empty runs, so that all RG_BLOCKS slots of the word are written.
template <int WORD>
__device__ __forceinline__ void mg_store_slot(double *slots, int64_t b, double s)
{
    if (threadIdx.x == 0) slots[(b * RG_BLOCKS + blockIdx.x) * 2 + WORD] = s;
    if (blockIdx.x == 0)
        for (int g = gridDim.x + threadIdx.x; g < RG_BLOCKS; g += BLOCK) slots[(b * RG_BLOCKS + g) * 2 + WORD] = 0.0;
}

// x = 0, r = g (through the batch stride gsb); word 1 = <g,g>
template <typename R>
__global__ __launch_bounds__(BLOCK) void mgcg_init(int64_t n, const R *__restrict__ g, int64_t gsb, R *__restrict__ x, R *__restrict__ r,
                                                   double *__restrict__ slots, int B)
{
    __shared__ double part[BLOCK / 64];
    int64_t lo, hi;
    run_of(n, blockIdx.x, lo, hi);
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        double acc = 0.0;
        for (int64_t i = lo + threadIdx.x; i < hi; i += BLOCK) {
            const R v = g[b * gsb + i];
            x[b * n + i] = R(0);
            r[b * n + i] = v;
            acc += (double)v * (double)v;
        }
        mg_store_slot<1>(slots, b, block_sum1(acc, part));
    }
}

// word 0 = <u,v>; COPY: p = v as well (the first direction)
template <typename R, bool COPY>
__global__ __launch_bounds__(BLOCK) void mgcg_dot(int64_t n, const R *__restrict__ u, const R *__restrict__ v, R *__restrict__ pp,
                                                  double *__restrict__ slots, int B)
{
    __shared__ double part[BLOCK / 64];
    int64_t lo, hi;
    run_of(n, blockIdx.x, lo, hi);
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        double acc = 0.0;
        for (int64_t i = lo + threadIdx.x; i < hi; i += BLOCK) {
            const R a = u[b * n + i], c = v[b * n + i];
            if (COPY) pp[b * n + i] = c;
            acc += (double)a * (double)c;
        }
        mg_store_slot<0>(slots, b, block_sum1(acc, part));
    }
}

// x += alpha p, r -= alpha q; word 1 = <r,r>.  A done item keeps its bits.
template <typename R>
__global__ __launch_bounds__(BLOCK) void mgcg_update(int64_t n, R *__restrict__ x, R *__restrict__ r, const R *__restrict__ pp,
                                                     const R *__restrict__ q, double *__restrict__ slots, const double *__restrict__ scal, int B)
{
    __shared__ double part[BLOCK / 64];
    int64_t lo, hi;
    run_of(n, blockIdx.x, lo, hi);
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        if (scal[b * S_STRIDE + S_DONE] != 0.0) {                   // (uniform per item)
            mg_store_slot<1>(slots, b, 0.0);
            continue;
        }
        const R alpha = (R)scal[b * S_STRIDE + S_ALPHA];
        double acc = 0.0;
        for (int64_t i = lo + threadIdx.x; i < hi; i += BLOCK) {
            const int64_t e = b * n + i;
            const R rv = fma_(-alpha, q[e], r[e]);
            x[e] = fma_(alpha, pp[e], x[e]);
            r[e] = rv;
            acc += (double)rv * (double)rv;
        }
        mg_store_slot<1>(slots, b, block_sum1(acc, part));
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------
struct Level {
    KParams k; WeightsEL<double> w; Diag<double> c; int mask; double s[3];
    const void *H; int64_t hbs;                                      // the Hessian of the level and its batch stride (elements)
    const void *r; int64_t rsb; void *a, *b;                         // the right-hand side, the two sweep buffers
};

// scal: the scalars of the items once solve_scalars<0> has written them (a done item is skipped), else NULL
struct Cycle { int nlev, mode, hk, B, Bh, nu, slide; Level lv[MG_MAX_LEVELS]; hipStream_t st; const double *scal; };

// the level shapes, tables and masks of a problem (no pointers yet); an error code of reg_weights, or 0
static int mg_levels(const KParams &k0, const double *wt, int slide, const double *voxel_size, int es, Cycle *cy)
{
    const int D = k0.dim;
    double h[3] = { 1, 1, 1 }, kappa = 1;
    for (int d = 0; d < D; ++d) h[d] = voxel_size[d];
    KParams k = k0;
    cy->nlev = 0;
    for (;;) {
        Level &l = cy->lv[cy->nlev];
        l.k = k;
        const int mode = reg_weights(D, kappa * wt[0], kappa * wt[1], kappa * wt[2], kappa * wt[3], kappa * wt[4], slide, h, &l.w);
        if (mode < 0) return mode;
        if (cy->nlev == 0) cy->mode = mode;
        else if (mode != cy->mode) return INTERPOL_E_SHAPE;         // (a weight that overflows or vanishes when scaled)
        solve_centre(l.w, mode, D, &l.c);
        l.mask = 0;
        for (int d = 0; d < 3; ++d) {
            l.s[d] = 1;
            if (d < D && k.vol_n[d] % 2 == 0 && k.vol_n[d] / 2 >= 4) { l.mask |= 1 << d; l.s[d] = 2; }
        }
        ++cy->nlev;
        if (!l.mask || cy->nlev == MG_MAX_LEVELS) { l.mask = 0; break; }
        int64_t N = 1, stride = D;
        for (int d = D - 1; d >= 0; --d) {
            if ((l.mask >> d) & 1) { k.vol_n[d] /= 2; k.gshape[d] = k.vol_n[d]; h[d] *= 2; kappa *= 2; }
            k.vol_ss[d] = (int)(stride * es);
            stride *= k.vol_n[d];
            N *= k.vol_n[d];
        }
        k.N = N;
    }
    return 0;
}

// bytes of the levels >= 1 (r, a, b and the Hessian each) behind `at`; sets the offsets when `off` is given
struct LevelOffsets { int64_t r, a, b, H; };
static int64_t mg_level_bytes(const Cycle &cy, int64_t B, int64_t Bh, int K, int64_t es, int64_t at, LevelOffsets *off)
{
    for (int l = 1; l < cy.nlev; ++l) {
        const int64_t field = align256(B * cy.lv[l].k.N * cy.lv[l].k.dim * es), hess = align256(Bh * cy.lv[l].k.N * K * es);
        if (off) { off[l].r = at; off[l].a = at + field; off[l].b = at + 2 * field; off[l].H = at + 3 * field; }
        at += 3 * field + hess;
    }
    return at;
}

template <typename R> static Diag<R> narrow_diag(const Diag<double> &c)
{
    Diag<R> r;
    for (int d = 0; d < 3; ++d) r.c[d] = (R)c.c[d];
    return r;
}

static dim3 point_grid(int64_t N, unsigned by) { return dim3((unsigned)((N + BLOCK - 1) / BLOCK), by, 1); }   // (N < 2^30)

template <typename R, int D, int MODE, int HK>
static void mg_apply_launch(const Cycle &cy, const Level &l, int op, const void *x, const void *r, int64_t rsb, void *out, unsigned by)
{
    hipLaunchKernelGGL((mg_apply<R, D, MODE, HK>), point_grid(l.k.N, by), dim3(BLOCK), 0, cy.st, l.k, WeightsOf<R, MODE>(narrow<R>(l.w)),
                       narrow_diag<R>(l.c), op, (const R *)x, (const R *)r, rsb, (const R *)l.H, l.hbs, (R *)out, cy.scal, cy.B);
}

template <typename R, int D, int MODE>
static void mg_apply_kind(const Cycle &cy, const Level &l, int op, const void *x, const void *r, int64_t rsb, void *out, unsigned by)
{
    switch (cy.hk) {
    case HK_NONE: return mg_apply_launch<R, D, MODE, HK_NONE>(cy, l, op, x, r, rsb, out, by);
    case HK_DIAG: return mg_apply_launch<R, D, MODE, HK_DIAG>(cy, l, op, x, r, rsb, out, by);
    default: return mg_apply_launch<R, D, MODE, HK_FULL>(cy, l, op, x, r, rsb, out, by);
    }
}

template <typename R, int D>
static void mg_apply_any(const Cycle &cy, const Level &l, int op, const void *x, const void *r, int64_t rsb, void *out, unsigned by)
{
    switch (cy.mode) {
    case 1: return mg_apply_kind<R, D, 1>(cy, l, op, x, r, rsb, out, by);
    case 2: return mg_apply_kind<R, D, 2>(cy, l, op, x, r, rsb, out, by);
    case 3: return mg_apply_kind<R, D, 3>(cy, l, op, x, r, rsb, out, by);
    case 4: return mg_apply_kind<R, D, 4>(cy, l, op, x, r, rsb, out, by);
    case 5: return mg_apply_kind<R, D, 5>(cy, l, op, x, r, rsb, out, by);
    case 6: return mg_apply_kind<R, D, 6>(cy, l, op, x, r, rsb, out, by);
    case 7: return mg_apply_kind<R, D, 7>(cy, l, op, x, r, rsb, out, by);
    case 10: return mg_apply_kind<R, D, 10>(cy, l, op, x, r, rsb, out, by);
    case 11: return mg_apply_kind<R, D, 11>(cy, l, op, x, r, rsb, out, by);
    case 14: return mg_apply_kind<R, D, 14>(cy, l, op, x, r, rsb, out, by);
    default: return mg_apply_kind<R, D, 15>(cy, l, op, x, r, rsb, out, by);
    }
}

template <typename R, int D>
static void mg_first_any(const Cycle &cy, const Level &l, unsigned by)
{
    const dim3 grid = point_grid(l.k.N, by);
    const Diag<R> c = narrow_diag<R>(l.c);
    switch (cy.hk) {
    case HK_NONE: hipLaunchKernelGGL((mg_first<R, D, HK_NONE>), grid, dim3(BLOCK), 0, cy.st, l.k.N, c, (const R *)l.r, l.rsb, (const R *)l.H, l.hbs, (R *)l.a, cy.scal, cy.B); break;
    case HK_DIAG: hipLaunchKernelGGL((mg_first<R, D, HK_DIAG>), grid, dim3(BLOCK), 0, cy.st, l.k.N, c, (const R *)l.r, l.rsb, (const R *)l.H, l.hbs, (R *)l.a, cy.scal, cy.B); break;
    default: hipLaunchKernelGGL((mg_first<R, D, HK_FULL>), grid, dim3(BLOCK), 0, cy.st, l.k.N, c, (const R *)l.r, l.rsb, (const R *)l.H, l.hbs, (R *)l.a, cy.scal, cy.B); break;
    }
}

// WHAT 0: restrict `fine` of level l to `coarse` of level l + 1; 1: prolong-and-add the other way
template <typename R, int D, int MASK, int WHAT>
static void mg_transfer_launch(const Cycle &cy, int l, const void *from, void *to, unsigned by)
{
    if constexpr (MASK < (1 << D)) {
        const Level &f = cy.lv[l], &c = cy.lv[l + 1];
        Scale<R> sc;
        for (int d = 0; d < 3; ++d) sc.s[d] = (R)f.s[d];
        if (WHAT == 0)
            hipLaunchKernelGGL((mg_restrict<R, D, MASK>), point_grid(c.k.N, by), dim3(BLOCK), 0, cy.st, c.k, f.k.vol_n[0], f.k.vol_n[1],
                               f.k.vol_n[2], cy.slide, sc, f.k.N, (const R *)from, (R *)to, cy.scal, cy.B);
        else
            hipLaunchKernelGGL((mg_prolong_add<R, D, MASK>), point_grid(f.k.N, by), dim3(BLOCK), 0, cy.st, f.k, c.k.vol_n[0], c.k.vol_n[1],
                               c.k.vol_n[2], cy.slide, sc, c.k.N, (const R *)from, (R *)to, cy.scal, cy.B);
    }
}

template <typename R, int D, int WHAT>
static void mg_transfer(const Cycle &cy, int l, const void *from, void *to, unsigned by)
{
    switch (cy.lv[l].mask) {
    case 1: return mg_transfer_launch<R, D, 1, WHAT>(cy, l, from, to, by);
    case 2: return mg_transfer_launch<R, D, 2, WHAT>(cy, l, from, to, by);
    case 3: return mg_transfer_launch<R, D, 3, WHAT>(cy, l, from, to, by);
    case 4: return mg_transfer_launch<R, D, 4, WHAT>(cy, l, from, to, by);
    case 5: return mg_transfer_launch<R, D, 5, WHAT>(cy, l, from, to, by);
    case 6: return mg_transfer_launch<R, D, 6, WHAT>(cy, l, from, to, by);
    default: return mg_transfer_launch<R, D, 7, WHAT>(cy, l, from, to, by);
    }
}

template <typename R, int D, int K, int MASK>
static void mg_hess_launch(const Cycle &cy, int l, unsigned by)
{
    if constexpr (MASK < (1 << D)) {
        const Level &f = cy.lv[l], &c = cy.lv[l + 1];
        Scale6<R> se;
        int i = 0;
        for (int d = 0; d < D; ++d) se.s[i++] = (R)(f.s[d] * f.s[d]);
        if (K > D)
            for (int d = 0; d < D; ++d)
                for (int e = d + 1; e < D; ++e) se.s[i++] = (R)(f.s[d] * f.s[e]);
        for (; i < 6; ++i) se.s[i] = R(0);
        hipLaunchKernelGGL((mg_coarsen_hess<R, D, K, MASK>), point_grid(c.k.N, by), dim3(BLOCK), 0, cy.st, c.k, f.k.vol_n[0], f.k.vol_n[1],
                           f.k.vol_n[2], se, (const R *)f.H, f.hbs, (R *)const_cast<void *>(c.H), cy.Bh);
    }
}

template <typename R, int D, int K>
static void mg_hess_mask(const Cycle &cy, int l, unsigned by)
{
    switch (cy.lv[l].mask) {
    case 1: return mg_hess_launch<R, D, K, 1>(cy, l, by);
    case 2: return mg_hess_launch<R, D, K, 2>(cy, l, by);
    case 3: return mg_hess_launch<R, D, K, 3>(cy, l, by);
    case 4: return mg_hess_launch<R, D, K, 4>(cy, l, by);
    case 5: return mg_hess_launch<R, D, K, 5>(cy, l, by);
    case 6: return mg_hess_launch<R, D, K, 6>(cy, l, by);
    default: return mg_hess_launch<R, D, K, 7>(cy, l, by);
    }
}

// the Hessian pyramid, once per call
template <typename R, int D>
static void mg_hessians(const Cycle &cy)
{
    if (cy.hk == HK_NONE) return;
    const unsigned by = (unsigned)(cy.Bh < 65535 ? cy.Bh : 65535);
    for (int l = 0; l + 1 < cy.nlev; ++l) {
        if (cy.hk == HK_DIAG) mg_hess_mask<R, D, D>(cy, l, by);
        else mg_hess_mask<R, D, D * (D + 1) / 2>(cy, l, by);
    }
}

// z = V(r) on level l; returns the buffer that holds it (level 0: always lv[0].b)
template <typename R, int D>
static void *mg_vcycle(const Cycle &cy, int l, unsigned by)
{
    const Level &lv = cy.lv[l];
    const bool last = l + 1 == cy.nlev;
    const int nu = last ? MG_COARSEST_SWEEPS : cy.nu;
    mg_first_any<R, D>(cy, lv, by);
    void *cur = lv.a, *other = lv.b;
    for (int s = 1; s < nu; ++s) {
        mg_apply_any<R, D>(cy, lv, 2, cur, lv.r, lv.rsb, other, by);
        void *t = cur; cur = other; other = t;
    }
    if (last) return cur;
    mg_apply_any<R, D>(cy, lv, 1, cur, lv.r, lv.rsb, other, by);                       // d, in the idle buffer
    mg_transfer<R, D, 0>(cy, l, other, const_cast<void *>(cy.lv[l + 1].r), by);
    const void *e = mg_vcycle<R, D>(cy, l + 1, by);
    mg_transfer<R, D, 1>(cy, l, e, cur, by);
    for (int s = 0; s < nu; ++s) {
        mg_apply_any<R, D>(cy, lv, 2, cur, lv.r, lv.rsb, other, by);
        void *t = cur; cur = other; other = t;
    }
    return cur;
}

struct MgSolve { const void *g; int64_t gsb; void *x, *r, *p, *q; double *slots, *scal, *info; int max_iter; double tol2; };

template <typename R, int D>
static void mg_solve_run(Cycle &cy, const MgSolve &a)
{
    const unsigned by = (unsigned)(cy.B < 65535 ? cy.B : 65535);
    const int64_t n = cy.lv[0].k.N * D;
    const int64_t chunk = ((n + RG_BLOCKS - 1) / RG_BLOCKS + BLOCK - 1) / BLOCK * BLOCK;      // (run_of's)
    const dim3 rgrid((unsigned)((n + chunk - 1) / chunk), by, 1), egrid((unsigned)((n + BLOCK - 1) / BLOCK), by, 1);
    mg_hessians<R, D>(cy);
    hipLaunchKernelGGL((mgcg_init<R>), rgrid, dim3(BLOCK), 0, cy.st, n, (const R *)a.g, a.gsb, (R *)a.x, (R *)a.r, a.slots, cy.B);
    const void *z = mg_vcycle<R, D>(cy, 0, by);
    hipLaunchKernelGGL((mgcg_dot<R, true>), rgrid, dim3(BLOCK), 0, cy.st, n, (const R *)a.r, (const R *)z, (R *)a.p, a.slots, cy.B);
    hipLaunchKernelGGL((solve_scalars<0>), dim3(by), dim3(BLOCK), 0, cy.st, (const double *)a.slots, a.scal, a.info, a.tol2, cy.B);
    cy.scal = a.scal;                                               // (from here on the done flags exist)
    for (int it = 0; it < a.max_iter; ++it) {
        mg_apply_any<R, D>(cy, cy.lv[0], 0, a.p, nullptr, 0, a.q, by);
        hipLaunchKernelGGL((mgcg_dot<R, false>), rgrid, dim3(BLOCK), 0, cy.st, n, (const R *)a.p, (const R *)a.q, (R *)nullptr, a.slots, cy.B);
        hipLaunchKernelGGL((solve_scalars<1>), dim3(by), dim3(BLOCK), 0, cy.st, (const double *)a.slots, a.scal, a.info, a.tol2, cy.B);
        hipLaunchKernelGGL((mgcg_update<R>), rgrid, dim3(BLOCK), 0, cy.st, n, (R *)a.x, (R *)a.r, (const R *)a.p, (const R *)a.q, a.slots,
                           (const double *)a.scal, cy.B);
        z = mg_vcycle<R, D>(cy, 0, by);
        hipLaunchKernelGGL((mgcg_dot<R, false>), rgrid, dim3(BLOCK), 0, cy.st, n, (const R *)a.r, (const R *)z, (R *)nullptr, a.slots, cy.B);
        hipLaunchKernelGGL((solve_scalars<2>), dim3(by), dim3(BLOCK), 0, cy.st, (const double *)a.slots, a.scal, a.info, a.tol2, cy.B);
        if (it + 1 < a.max_iter)                                    // (the direction after the last update moves nothing in x)
            hipLaunchKernelGGL((solve_direction<R>), egrid, dim3(BLOCK), 0, cy.st, n, (const R *)z, (R *)a.p, (const double *)a.scal, cy.B);
    }
}

template <typename R, int D>
static void mg_cycle_run(Cycle &cy)
{
    mg_hessians<R, D>(cy);
    mg_vcycle<R, D>(cy, 0, (unsigned)(cy.B < 65535 ? cy.B : 65535));
}

template <typename R>
static void mg_by_dim(Cycle &cy, const MgSolve *a)
{
    switch (cy.lv[0].k.dim) {
    case 1: return a ? mg_solve_run<R, 1>(cy, *a) : mg_cycle_run<R, 1>(cy);
    case 2: return a ? mg_solve_run<R, 2>(cy, *a) : mg_cycle_run<R, 2>(cy);
    default: return a ? mg_solve_run<R, 3>(cy, *a) : mg_cycle_run<R, 3>(cy);
    }
}

// the workspace of the solve: r, p, q, a_0, z (B, N, D) each, the slots, the scalars, then level by level r_l, a_l, b_l and H_l;
// of the cycle alone: a_0, then the levels.  Every part starts at a multiple of 256 bytes from the base.
struct MgLayout { int64_t r, p, q, a, z, slots, scal, levels, total; };

static MgLayout mg_layout(const Cycle &cy, int64_t B, int64_t Bh, int K, int64_t es, bool solve)
{
    const KParams &k = cy.lv[0].k;
    const int64_t field = align256(B * k.N * k.dim * es);
    MgLayout l;
    memset(&l, 0, sizeof(l));
    if (solve) {
        l.r = 0; l.p = field; l.q = 2 * field; l.a = 3 * field; l.z = 4 * field; l.slots = 5 * field;
        l.scal = l.slots + align256(B * RG_BLOCKS * 2 * (int64_t)sizeof(double));
        l.levels = l.scal + align256(B * S_STRIDE * (int64_t)sizeof(double));
    } else {
        l.a = 0; l.levels = field;
    }
    l.total = mg_level_bytes(cy, B, Bh, K, es, l.levels, nullptr);
    return l;
}

static const double MG_UNIT_WEIGHTS[5] = { 1, 0, 0, 0, 0 }, MG_UNIT_VOXELS[3] = { 1, 1, 1 };

// the size query: the levels depend on the shape alone, and the pyramid is sized for a Hessian per item
static int64_t mg_workspace(const interpol_problem *p, int hessian_components, bool solve)
{
    Cycle cy;
    int B, slide;
    KParams k;
    int rc = solve_params(p, &k, &B, &slide);
    if (rc) return rc;
    const int hk = hess_kind(k.dim, hessian_components);
    if (hk < 0) return hk;
    const int es = p->dtype == INTERPOL_F64 ? 8 : 4;
    rc = mg_levels(k, MG_UNIT_WEIGHTS, 0, MG_UNIT_VOXELS, es, &cy);
    if (rc) return rc;
    return mg_layout(cy, B, B, hessian_components, es, solve).total;
}

// both entry points: `solution` is x (solve) or z (cycle); the cycle has max_iter = -1 and no info
static int mg_entry(const interpol_problem *p, const void *gradient, const void *hessian, int hessian_components,
                    int64_t hessian_batch_stride, void *solution, const double *wt, const double *voxel_size, int smoothing, bool solve,
                    int max_iter, double tolerance, void *info, void *workspace, int64_t workspace_bytes, void *stream)
{
    Cycle c;
    KParams k;
    int slide = 0;
    int rc = solve_params(p, &k, &c.B, &slide);
    if (rc) return rc;
    if (!wt || !voxel_size) return INTERPOL_E_NULL;
    WeightsEL<double> w0;
    const int mode = reg_weights(k.dim, wt[0], wt[1], wt[2], wt[3], wt[4], slide, voxel_size, &w0);
    if (mode < 0) return mode;
    if (!reg_symmetric(k, slide, wt[3] > 0 || wt[4] > 0)) return INTERPOL_E_BOUND;
    c.hk = hess_kind(k.dim, hessian_components);
    if (c.hk < 0) return c.hk;
    if (smoothing < 1 || smoothing > 1024) return INTERPOL_E_SHAPE;
    if (solve && (max_iter < 0 || !(tolerance >= 0) || !(tolerance < 1e150))) return INTERPOL_E_SHAPE;
    if (hessian_batch_stride < 0) return INTERPOL_E_STRIDE;
    if (!gradient || !solution || !workspace || (c.hk != HK_NONE && !hessian)) return INTERPOL_E_NULL;
    const int D = k.dim;
    const int64_t B = c.B;
    const int64_t es = p->dtype == INTERPOL_F64 ? 8 : 4;
    rc = mg_levels(k, wt, slide, voxel_size, (int)es, &c);
    if (rc) return rc;
    c.slide = slide;                                                // (the grid transfers: per component under every weight set)
    c.nu = smoothing;
    c.st = (hipStream_t)stream;
    c.scal = nullptr;
    c.Bh = c.hk == HK_NONE ? 0 : (hessian_batch_stride == 0 ? 1 : (int)B);
    if ((uintptr_t)workspace % sizeof(double)) return INTERPOL_E_STRIDE;
    const MgLayout l = mg_layout(c, B, c.Bh, hessian_components, es, solve);
    if (workspace_bytes < l.total) return INTERPOL_E_SCRATCH;
    const uint64_t item = (uint64_t)k.N * D * es;
    const uint64_t gspan = (uint64_t)(B - 1) * (uint64_t)k.vol_sb * es + item;
    const uint64_t hitem = (uint64_t)k.N * hessian_components * es;
    const uint64_t hspan = c.hk == HK_NONE ? 0 : (uint64_t)(B - 1) * (uint64_t)hessian_batch_stride * es + hitem;
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
    char *ws = (char *)workspace;
    LevelOffsets off[MG_MAX_LEVELS];
    mg_level_bytes(c, B, c.Bh, hessian_components, es, l.levels, off);
    Level &l0 = c.lv[0];
    l0.H = hessian; l0.hbs = c.hk == HK_NONE ? 0 : hessian_batch_stride;            // (no Hessian: never dereferenced)
    l0.a = ws + l.a;
    if (solve) { l0.r = ws + l.r; l0.rsb = k.N * D; l0.b = ws + l.z; }
    else { l0.r = gradient; l0.rsb = k.vol_sb; l0.b = solution; }
    for (int i = 1; i < c.nlev; ++i) {
        Level &li = c.lv[i];
        li.r = ws + off[i].r; li.rsb = li.k.N * D; li.a = ws + off[i].a; li.b = ws + off[i].b;
        li.H = ws + off[i].H; li.hbs = c.Bh > 1 ? li.k.N * hessian_components : 0;
    }
    MgSolve a;
    a.g = gradient; a.gsb = k.vol_sb; a.x = solution; a.r = ws + l.r; a.p = ws + l.p; a.q = ws + l.q;
    a.slots = (double *)(ws + l.slots); a.scal = (double *)(ws + l.scal); a.info = (double *)info;
    a.max_iter = max_iter; a.tol2 = tolerance * tolerance;
    if (p->dtype == INTERPOL_F64) mg_by_dim<double>(c, solve ? &a : nullptr);
    else mg_by_dim<float>(c, solve ? &a : nullptr);
    return hipGetLastError() == hipSuccess ? 0 : INTERPOL_E_LAUNCH;
}

} // namespace reg
} // namespace ip

extern "C" {

int64_t interpol_regulariser_multigrid_solve_workspace(const interpol_problem *p, int hessian_components)
{
    return ip::reg::mg_workspace(p, hessian_components, true);
}

int interpol_regulariser_multigrid_solve(const interpol_problem *p, const void *gradient, const void *hessian, int hessian_components,
                                         int64_t hessian_batch_stride, void *solution, const double *weights, const double *voxel_size,
                                         int smoothing, int max_iter, double tolerance, void *info, void *workspace,
                                         int64_t workspace_bytes, void *stream)
{
    return ip::reg::mg_entry(p, gradient, hessian, hessian_components, hessian_batch_stride, solution, weights, voxel_size, smoothing,
                             true, max_iter, tolerance, info, workspace, workspace_bytes, stream);
}

int64_t interpol_regulariser_multigrid_cycle_workspace(const interpol_problem *p, int hessian_components)
{
    return ip::reg::mg_workspace(p, hessian_components, false);
}

int interpol_regulariser_multigrid_cycle(const interpol_problem *p, const void *residual, const void *hessian, int hessian_components,
                                         int64_t hessian_batch_stride, void *out, const double *weights, const double *voxel_size,
                                         int smoothing, void *workspace, int64_t workspace_bytes, void *stream)
{
    return ip::reg::mg_entry(p, residual, hessian, hessian_components, hessian_batch_stride, out, weights, voxel_size, smoothing,
                             false, -1, 0.0, nullptr, workspace, workspace_bytes, stream);
}

} // extern "C"
