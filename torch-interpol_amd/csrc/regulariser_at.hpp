// ===========================================================================
// regulariser_at.hpp -- what the kernels of the smoothness penalty share: the stencil of L at one lattice point (reg_at), its
// coefficient tables, the fixed-order workgroup sum and the host-side validation.  Included by regulariser.hip (L v and the
// energy) and by regulariser_solve.hip (the conjugate-gradient solve of (H + L) x = g); the definitions are in regulariser.hip's
// header comment.
// ===========================================================================
#pragma once
#include "../../include/interpol_hip.h"
#include "ops_generic.hpp"
#include <hip/hip_runtime.h>
#include <string.h>

namespace ip {
namespace reg {

// Persistent workgroups of reg_energy per batch item = doubles per item in the workspace.  A CONSTANT (see above).
constexpr int RG_BLOCKS = 1024;

// M_EL: the linear-elastic terms, and / or a sliding dimension (per-component signs).  The host sets M_MEM with it (shears
// folds into the per-axis membrane weights), so the modes are 1..7 and 10, 11, 14, 15.
enum { M_ABS = 1, M_MEM = 2, M_BEND = 4, M_EL = 8 };

// D components of one lattice point; alignment of a single component (as in jacobian.hip)
template <typename R, int D> struct PointVec { R c[D]; };
static_assert(alignof(PointVec<float, 3>) == 4 && sizeof(PointVec<float, 3>) == 12, "point-by-point element: 4-byte aligned");

// The coefficient tables, combined on the host in double and rounded once (a_d = 1 / h_d^2):
//   axis[d][k] : weight of the taps at distance k along d in  membrane A_d + bending B_d  -- k = 0: 2 m a + 6 b a^2,
//                k = 1: -m a - 4 b a^2, k = 2: b a^2
//   a1[d][k]   : the taps of A_d alone, 2 a and -a (the factors of the mixed terms)
//   bend2      : 2 bending (sum_{e != f} = 2 sum_{e < f}),  h2[d] = h_d^2
template <typename R> struct Weights { R abs, bend2; R axis[3][3]; R a1[3][2]; R h2[3]; };
// what the M_EL modes take on top (shears is part of the membrane weight m of axis[][] then); the kernels of the other modes
// take Weights alone, as they did:
//   axo[d][k]  : axis[d][k] plus the own-axis extra (shears + div) a (2, -1, 0) -- the taps of component d along d
//   cross      : -(shears + div) / 4, the one coefficient of the diagonal taps of X_ce (no voxel size: h_c h_e cancels)
//   slide      : bit d = dimension d is sliding (indexed as dct2; component d takes the signs of dst2 along d)
template <typename R> struct WeightsEL : Weights<R> { R axo[3][3]; R cross; int slide; };
template <typename R, int MODE> struct WeightsPick { typedef Weights<R> type; };
template <typename R> struct WeightsPick<R, 10> { typedef WeightsEL<R> type; };
template <typename R> struct WeightsPick<R, 11> { typedef WeightsEL<R> type; };
template <typename R> struct WeightsPick<R, 14> { typedef WeightsEL<R> type; };
template <typename R> struct WeightsPick<R, 15> { typedef WeightsEL<R> type; };
template <typename R, int MODE> using WeightsOf = typename WeightsPick<R, MODE>::type;

template <int D>
__device__ __forceinline__ void split_index(const KParams &p, int64_t o, unsigned *od)
{
    unsigned r = (unsigned)o;                                        // (N < 2^30: one item of the field spans < 4 GiB)
#pragma unroll
    for (int d = D - 1; d > 0; --d) { const unsigned q = r / (unsigned)p.gshape[d]; od[d] = r - q * (unsigned)p.gshape[d]; r = q; }
    od[0] = r;
}

// out[c] = (L v)_c at the lattice point od of one batch item `ub`; v0: the field at that point.  The field is stored in R; the
// coefficients, the products and the sum are formed in A (A = R everywhere but in the energy of a float32 field, which takes double:
// the stencil of a smooth field cancels, and an energy is compared relative to itself)
template <typename R, int D, int MODE, typename A = R>
__device__ __forceinline__ void reg_at(const KParams &p, const WeightsOf<A, MODE> &w, const PointVec<R, D> *ub, const unsigned *od,
                                       PointVec<R, D> &v0, A (&out)[D])
{
    typedef PointVec<R, D> V;
    constexpr bool ABS = (MODE & M_ABS) != 0, MEM = (MODE & M_MEM) != 0, BEND = (MODE & M_BEND) != 0, EL = (MODE & M_EL) != 0;
    static_assert(!EL || MEM, "the elastic modes carry the membrane bit");
    constexpr int RAD = BEND ? 2 : (MEM ? 1 : 0);
    constexpr int T = 2 * RAD + 1;
    unsigned cen = 0;
#pragma unroll
    for (int d = 0; d < D; ++d) cen += od[d] * (unsigned)p.vol_ss[d];
    v0 = ld_tap(ub, cen);
    if (RAD == 0) {
#pragma unroll
        for (int c = 0; c < D; ++c) out[c] = w.h2[c] * (w.abs * (A)v0.c[c]);
        return;
    }
    unsigned off[D][T];
    A wm[D][T], wa[D][3];
    // M_EL only: the same for component d along its own axis d, and the signed +-1 of the two distance-1 taps (xs: any component, xso: d)
    A wmo[D][T], wao[D][3], xs[D][2], xso[D][2];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const int n = p.vol_n[d], bd = p.bound[d], i0 = (int)od[d] - RAD;
        int idx[T], sg[T], so[T];
        // the inside test of Stencil::setup over the 2 RAD + 1 taps (dst1: the sign is 0 at index 0)
        const bool inside = i0 >= (bd == B_DST1 ? 1 : 0) && i0 + T - 1 < n;
#pragma unroll
        for (int j = 0; j < T; ++j) { idx[j] = i0 + j; sg[j] = 1; }
        if (!inside) {
#pragma unroll
            for (int j = 0; j < T; ++j) {
                const long long pk = wrap_outofline(bd, i0 + j, n);
                idx[j] = (int)(pk & 0xffffffffll);
                sg[j]  = (int)(pk >> 32);
            }
        }
        if constexpr (EL) {
#pragma unroll
            for (int j = 0; j < T; ++j) so[j] = sg[j];
            // a sliding dimension (bd is dct2): its own component takes the signs of dst2, which has the same index map
            if (!inside && ((w.slide >> d) & 1)) {
#pragma unroll
                for (int j = 0; j < T; ++j) so[j] = (int)(wrap_outofline(B_DST2, i0 + j, n) >> 32);
            }
        }
#pragma unroll
        for (int j = 0; j < T; ++j) {
            const int k = j < RAD ? RAD - j : j - RAD;
            off[d][j] = (unsigned)idx[j] * (unsigned)p.vol_ss[d];
            wm[d][j] = w.axis[d][k] * A(sg[j]);
            if constexpr (EL) wmo[d][j] = w.axo[d][k] * A(so[j]);
        }
#pragma unroll
        for (int t = 0; t < 3; ++t) wa[d][t] = w.a1[d][t == 1 ? 0 : 1] * A(sg[RAD - 1 + t]);
        if constexpr (EL) {
#pragma unroll
            for (int t = 0; t < 3; ++t) wao[d][t] = w.a1[d][t == 1 ? 0 : 1] * A(so[RAD - 1 + t]);
            xs[d][0] = -A(sg[RAD - 1]); xs[d][1] = A(sg[RAD + 1]);
            xso[d][0] = -A(so[RAD - 1]); xso[d][1] = A(so[RAD + 1]);
        }
    }
    constexpr bool MIX = BEND && D > 1;
    // the centre: every term has a tap there
    A c0 = ABS ? w.abs : A(0);
#pragma unroll
    for (int d = 0; d < D; ++d) c0 += wm[d][RAD];
    if (MIX) {
        A pr = A(0);
#pragma unroll
        for (int e = 0; e < D; ++e) {
#pragma unroll
            for (int f = e + 1; f < D; ++f) pr = fma_(wa[e][1], wa[f][1], pr);
        }
        c0 = fma_(w.bend2, pr, c0);
    }
    A acc[D];
#pragma unroll
    for (int c = 0; c < D; ++c) {
        A cc = c0;
        if constexpr (EL) cc = c0 - wm[c][RAD] + wmo[c][RAD];            // (component c has its own centre tap along c)
        acc[c] = cc * (A)v0.c[c];
    }
    // along the axes: A_e and B_e, and at distance 1 the mixed terms A_e (x) centre of A_f
#pragma unroll
    for (int e = 0; e < D; ++e) {
        const unsigned rest = cen - off[e][RAD];
        A side = A(0);
        if (MIX) {
#pragma unroll
            for (int f = 0; f < D; ++f) if (f != e) side += wa[f][1];
            side *= w.bend2;
        }
#pragma unroll
        for (int j = 0; j < T; ++j) {
            if (j == RAD) continue;
            A coef = wm[e][j];
            if (MIX && (j == RAD - 1 || j == RAD + 1)) coef = fma_(side, wa[e][j - RAD + 1], coef);
            const V v = ld_tap(ub, rest + off[e][j]);
            if constexpr (EL) {
                A own = wmo[e][j];
                if (MIX && (j == RAD - 1 || j == RAD + 1)) own = fma_(side, wao[e][j - RAD + 1], own);
#pragma unroll
                for (int c = 0; c < D; ++c) acc[c] = fma_(c == e ? own : coef, (A)v.c[c], acc[c]);
                continue;
            }
#pragma unroll
            for (int c = 0; c < D; ++c) acc[c] = fma_(coef, (A)v.c[c], acc[c]);
        }
    }
    // the in-plane diagonals: with M_EL the cross-component taps of X_ce, and the mixed bending terms with per-component
    // signs, through ONE load per point
    if constexpr (EL && D > 1) {
        A xacc[D];
#pragma unroll
        for (int c = 0; c < D; ++c) xacc[c] = A(0);
        // (uniform: the three old terms under sliding have no cross term, and without bending no tap on the diagonals at all)
        if (MIX || w.cross != A(0)) {
#pragma unroll
        for (int e = 0; e < D; ++e) {
#pragma unroll
            for (int f = e + 1; f < D; ++f) {
                const unsigned rest = cen - off[e][RAD] - off[f][RAD];
#pragma unroll
                for (int t = 0; t < 3; t += 2) {
#pragma unroll
                    for (int u = 0; u < 3; u += 2) {
                        const V v = ld_tap(ub, rest + off[e][RAD - 1 + t] + off[f][RAD - 1 + u]);
                        // component f is extended by its own rule along f and by the common one along e, and e likewise
                        xacc[e] = fma_(xs[e][t / 2] * xso[f][u / 2], (A)v.c[f], xacc[e]);
                        xacc[f] = fma_(xso[e][t / 2] * xs[f][u / 2], (A)v.c[e], xacc[f]);
                        if (MIX) {
                            const A cg = w.bend2 * (wa[e][t] * wa[f][u]);
                            const A ce = w.bend2 * (wao[e][t] * wa[f][u]), cf = w.bend2 * (wa[e][t] * wao[f][u]);
#pragma unroll
                            for (int c = 0; c < D; ++c) acc[c] = fma_(c == e ? ce : (c == f ? cf : cg), (A)v.c[c], acc[c]);
                        }
                    }
                }
            }
        }
        }
#pragma unroll
        for (int c = 0; c < D; ++c) out[c] = fma_(w.cross, xacc[c], w.h2[c] * acc[c]);
        return;
    }
    // the in-plane diagonals of the mixed terms
    if (MIX) {
#pragma unroll
        for (int e = 0; e < D; ++e) {
#pragma unroll
            for (int f = e + 1; f < D; ++f) {
                const unsigned rest = cen - off[e][RAD] - off[f][RAD];
#pragma unroll
                for (int t = 0; t < 3; t += 2) {
#pragma unroll
                    for (int u = 0; u < 3; u += 2) {
                        const A coef = w.bend2 * (wa[e][t] * wa[f][u]);
                        const V v = ld_tap(ub, rest + off[e][RAD - 1 + t] + off[f][RAD - 1 + u]);
#pragma unroll
                        for (int c = 0; c < D; ++c) acc[c] = fma_(coef, (A)v.c[c], acc[c]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < D; ++c) out[c] = w.h2[c] * acc[c];
}

// sum of `acc` over the workgroup in a fixed order: lanes by halving shuffles, then the waves one after the other
// (block_sum of affine_grad.hip for one value); valid in every thread on return, `part` reusable after it
__device__ __forceinline__ double block_sum1(double acc, double *part)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    double s = part[0];
    for (int w = 1; w < BLOCK / 64; ++w) s += part[w];
    __syncthreads();
    return s;
}

// ---- host side --------------------------------------------------------------------------------------------------------
// Validate + convert (the conventions of jac_params, without an order): vol_* is the field, val_stride[0] the batch stride of
// L v, whose items are dense (energy: unused).
// `slide`: NULL for the three-term entry points (a bound above 6 is an error), else receives the mask of the dimensions
// whose bound is INTERPOL_BOUND_SLIDING; the kernels see dct2 there.
static int reg_params(const interpol_problem *p, bool with_out, KParams *k, int *B, int *slide = nullptr)
{
    if (!p) return INTERPOL_E_NULL;
    if (p->abi_version != INTERPOL_ABI_VERSION) return INTERPOL_E_SHAPE;
    if (p->dim < 1 || p->dim > 3) return INTERPOL_E_DIM;
    if (p->dtype != INTERPOL_F32 && p->dtype != INTERPOL_F64) return INTERPOL_E_DTYPE;
    if (p->batch < 1 || p->batch > 0x7fffffff || p->channels != p->dim) return INTERPOL_E_SHAPE;
    const int D = p->dim;
    const uint64_t es = p->dtype == INTERPOL_F64 ? 8 : 4;
    memset(k, 0, sizeof(*k));
    if (slide) *slide = 0;
    k->dim = D;
    k->extrapolate = 1;                                             // lattice points are in bounds
    for (int d = 0; d < D; ++d) {
        if (p->bound[d] < 0 || p->bound[d] > (slide ? INTERPOL_BOUND_SLIDING : 6)) return INTERPOL_E_BOUND;
        if (p->vol_shape[d] < 1 || p->vol_shape[d] > 0x3fffffff) return INTERPOL_E_SHAPE;
    }
    if (D > 1 && p->vol_stride[1] != 1) return INTERPOL_E_STRIDE;   // row-major, point by point
    int64_t exp = D, N = 1;
    uint64_t bytes = (uint64_t)D * es;
    for (int d = D - 1; d >= 0; --d) {
        if (p->vol_shape[d] > 1 && p->vol_stride[2 + d] != exp) return INTERPOL_E_STRIDE;
        k->vol_ss[d] = (int)((uint64_t)exp * es);                   // (< 2^32: one item of the field is, below)
        bytes *= (uint64_t)p->vol_shape[d];
        if (bytes > 0xffffffffull) return INTERPOL_E_SHAPE;         // one item of the field must fit 32-bit byte offsets
        exp *= p->vol_shape[d];
        N *= p->vol_shape[d];
    }
    if (p->vol_stride[0] < 0) return INTERPOL_E_STRIDE;
    if (with_out) {
        if (p->val_stride[0] < 0) return INTERPOL_E_STRIDE;
        if (p->batch > 1 && p->val_stride[0] < N * D) return INTERPOL_E_STRIDE;   // the output has an item of its own per batch item
    }
    for (int d = 0; d < 3; ++d) {
        if (d >= D) { k->bound[d] = 1; k->vol_n[d] = 1; k->vol_ss[d] = 0; k->gshape[d] = 1; continue; }
        k->bound[d] = p->bound[d];
        if (slide && p->bound[d] == INTERPOL_BOUND_SLIDING) { k->bound[d] = B_DCT2; *slide |= 1 << d; }
        k->vol_n[d] = (int)p->vol_shape[d];
        k->gshape[d] = (int)p->vol_shape[d];
    }
    k->C = D;
    k->N = N;
    k->vol_sb = p->vol_stride[0];
    k->vol_sc = 1;
    k->val_sb = with_out ? p->val_stride[0] : 0;
    k->val_sc = 1;
    *B = (int)p->batch;
    return 0;
}

// weights and voxel sizes -> the mode and the coefficient tables (double); INTERPOL_E_SHAPE for a negative or non-finite
// weight, a non-positive voxel size, or no term at all.  shears, div: the elastic weights; slide: the mask of reg_params.
// Without elastic weights and without a sliding dimension that moves a tap (absolute alone has none) the mode and the
// tables are those of the three-term operator, bit for bit.
static int reg_weights(int D, double absolute, double membrane, double bending, double shears, double div, int slide,
                       const double *voxel_size, WeightsEL<double> *w)
{
    if (!voxel_size) return INTERPOL_E_NULL;
    if (!(absolute >= 0 && membrane >= 0 && bending >= 0 && shears >= 0 && div >= 0)
        || !(absolute + membrane + bending + shears + div < 1e300)) return INTERPOL_E_SHAPE;
    int mode = (absolute > 0 ? M_ABS : 0) | (membrane > 0 ? M_MEM : 0) | (bending > 0 ? M_BEND : 0);
    const bool elastic = shears > 0 || div > 0;
    if (elastic || (slide && (mode & (M_MEM | M_BEND)))) mode |= M_EL | M_MEM;
    if (!mode) return INTERPOL_E_SHAPE;
    memset(w, 0, sizeof(*w));
    w->abs = absolute;
    w->bend2 = 2 * bending;
    w->cross = -(shears + div) / 4;
    w->slide = (mode & M_EL) ? slide : 0;
    const double m = elastic ? membrane + shears : membrane;         // (the three-term tables: untouched arithmetic)
    for (int d = 0; d < D; ++d) {
        const double h = voxel_size[d];
        if (!(h > 0) || !(h < 1e300)) return INTERPOL_E_SHAPE;
        const double a = 1 / (h * h);
        w->h2[d] = h * h;
        w->axis[d][0] = 2 * m * a + 6 * bending * a * a;
        w->axis[d][1] = -m * a - 4 * bending * a * a;
        w->axis[d][2] = bending * a * a;
        w->a1[d][0] = 2 * a;
        w->a1[d][1] = -a;
        w->axo[d][0] = 2 * (m + shears + div) * a + 6 * bending * a * a;
        w->axo[d][1] = -(m + shears + div) * a - 4 * bending * a * a;
        w->axo[d][2] = w->axis[d][2];
    }
    return mode;
}

// is L symmetric (what conjugate gradients need)?  k->bound after reg_params: a sliding dimension reads dct2 and has its
// bit in `slide`.  The three terms: zero, dct2, dst2, dft, sliding; with elastic weights: zero, dft, sliding.
static bool reg_symmetric(const KParams &k, int slide, bool elastic)
{
    for (int d = 0; d < k.dim; ++d) {
        const int b = k.bound[d];
        if (b == B_ZERO || b == B_DFT || ((slide >> d) & 1)) continue;
        if (!elastic && (b == B_DCT2 || b == B_DST2)) continue;
        return false;
    }
    return true;
}

template <typename R> static WeightsEL<R> narrow(const WeightsEL<double> &w)
{
    WeightsEL<R> r;
    r.abs = (R)w.abs; r.bend2 = (R)w.bend2; r.cross = (R)w.cross; r.slide = w.slide;
    for (int d = 0; d < 3; ++d) {
        r.h2[d] = (R)w.h2[d];
        for (int k = 0; k < 3; ++k) { r.axis[d][k] = (R)w.axis[d][k]; r.axo[d][k] = (R)w.axo[d][k]; }
        for (int k = 0; k < 2; ++k) r.a1[d][k] = (R)w.a1[d][k];
    }
    return r;
}

// do the byte ranges [a, a + na) and [b, b + nb) intersect?
static bool ranges_overlap(const void *a, uint64_t na, const void *b, uint64_t nb)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}

} // namespace reg
} // namespace ip
