// ===========================================================================
// data_term.hpp -- what the fused registration data terms share (ssd.hip, lcc.hip on a dense displacement field; ssd_affine.hip,
// mi_affine.hip, lcc_affine.hip on the matrix of an affine lattice, through affine_sums.hpp):
//
//   problem_params          : the validation of the problem and its conversion to KParams, by the kind of lattice
//   ranges_alias            : "what is written overlaps neither an input nor another output"
//   moving_bytes, fixed_bytes, weight_bytes : the bytes a call reads of its images, for ranges_alias
//   HK_*, hess_components, diag_first_index, pair_index : the two layouts of a symmetric D x D block
//   IP_STENCIL_VALUE_GRADIENT, stencil_value_gradient : one channel under a stencil in R: the value and the D derivative sums
//   IP_STENCIL_VALUE        : one channel under a stencil in double: the value
//   slot_finish<R>          : the kernel that sums an item's slots of doubles in a fixed order into its loss
//   dispatch                : dtype, dim 1..3 and order 1..3 from run-time values to template arguments
//
// A data term supplies its per-sample terms, the layout of its workspace and the checks of its own arguments.
// ===========================================================================
#pragma once
#include "../../include/interpol_hip.h"
#include "regulariser_at.hpp"                                      // ops_generic.hpp (Stencil, KParams), block_sum1, ranges_overlap
#include <hip/hip_runtime.h>
#include <string.h>
#include <type_traits>

namespace ip {
namespace dt {

// ---- the Hessian of a sample: two layouts of the upper triangle of a symmetric D x D block, both in use on purpose ----------------
//   diag_first_index : the diagonal first, then the strict upper triangle row by row -- the fields of ssd.hip and lcc.hip, which
//                      regulariser_solve.hip takes: a diagonal Hessian (HK_DIAG) is a prefix of the full one (HK_FULL).
//   pair_index       : the upper triangle with its diagonal, row by row -- the sums of affine_sums.hpp, where (d, d') and the
//                      moments (e, e') are indexed alike and nothing is ever a prefix.
enum { HK_NONE = 0, HK_DIAG = 1, HK_FULL = 2 };
constexpr int hess_components(int D, int hk) { return hk == HK_NONE ? 0 : (hk == HK_DIAG ? D : D * (D + 1) / 2); }
// index of (d, e), d < e < D, behind the D diagonal entries; (d, d) is at d
__host__ __device__ constexpr int diag_first_index(int d, int e, int D) { return D + d * D - d * (d + 1) / 2 + (e - d - 1); }
// index of (i, j), i <= j < n, in the upper triangle of an n x n matrix, row by row
__host__ __device__ constexpr int pair_index(int i, int j, int n) { return i * n - i * (i - 1) / 2 + (j - i); }

// ---- the stencil loops ------------------------------------------------------------------------------------------------------
// Written once, as macros in the manner of IP_FOR_I (ops_generic.hpp; R, D, KMAX and `p` come from the scope they expand in), because
// ssd_fwd and lcc_pull hold their Stencil as a local of the kernel: handed by reference to an inlined function it is taken
// apart after the inlining instead of before it, and the same operations come out under other register assignments (ssd_fwd<double,
// 3, 3, 0>: 135 VGPRs where the loop expanded in place takes 127, a wave per SIMD less).  Expanded in place each kernel is instruction
// for instruction what it was (profiles/data_term_refactor.txt).  Neither macro makes the offsets opaque: the call site does, where
// it has a channel loop to keep them out of (ops_generic.hpp: opaque).
//
// One channel at `v0` under the Stencil<R, D, KMAX, true, NEED_G> `s`, before the mask: aw += sum_taps W v, a0, a1, a2 += sum_taps
// dW/dx_d v (a1, a2 untouched for D < 2, 3).  A caller that does not read `aw` leaves its sum to dead-code elimination.
#define IP_STENCIL_VALUE_GRADIENT(s, v0, aw, a0, a1, a2)                                                                            \
    IP_FOR_I {                                                                                                                     \
        R pWW = R(0), pGW = R(0), pWG = R(0);                                                                                      \
        IP_FOR_J {                                                                                                                 \
            const unsigned oij = s.off[0][i] + s.off[1][j];                                                                        \
            R rW = R(0), rG = R(0);                                                                                                \
            IP_FOR_K {                                                                                                             \
                const R v = ld_tap(v0, oij + s.off[2][k]);                                                                         \
                rW = fma_(s.w[2][k], v, rW);                                                                                       \
                if (D > 2) rG = fma_(s.g[2][k], v, rG);                                                                            \
            } IP_ROW_END;                                                                                                          \
            pWW = fma_(s.w[1][j], rW, pWW);                                                                                        \
            if (D > 1) pGW = fma_(s.g[1][j], rW, pGW);                                                                             \
            if (D > 2) pWG = fma_(s.w[1][j], rG, pWG);                                                                             \
        }                                                                                                                          \
        aw = fma_(s.w[0][i], pWW, aw);                                                                                             \
        a0 = fma_(s.g[0][i], pWW, a0);                                                                                             \
        if (D > 1) a1 = fma_(s.w[0][i], pGW, a1);                                                                                  \
        if (D > 2) a2 = fma_(s.w[0][i], pWG, a2);                                                                                  \
    }

// One channel at `v0` under the Stencil<double, D, KMAX, true, NEED_W> `s`, before the mask: aw += sum_taps W v in double.
#define IP_STENCIL_VALUE(s, v0, aw)                                                                                                 \
    IP_FOR_I {                                                                                                                     \
        double pW = 0.0;                                                                                                           \
        IP_FOR_J {                                                                                                                 \
            const unsigned oij = s.off[0][i] + s.off[1][j];                                                                        \
            double rW = 0.0;                                                                                                       \
            IP_FOR_K {                                                                                                             \
                rW = fma_(s.w[2][k], (double)ld_tap(v0, oij + s.off[2][k]), rW);                                                   \
            } IP_ROW_END;                                                                                                          \
            pW = fma_(s.w[1][j], rW, pW);                                                                                          \
        }                                                                                                                          \
        aw = fma_(s.w[0][i], pW, aw);                                                                                              \
    }

// IP_STENCIL_VALUE_GRADIENT for the per-sample terms that are functions already (ssd_affine.hip, mi_affine.hip), inside a channel
// loop: the offsets are made opaque first.  aw = sum_taps W v, av[d] = sum_taps dW/dx_d v.
template <typename R, int D, int KMAX>
__device__ __forceinline__ void stencil_value_gradient(const KParams &p, Stencil<R, D, KMAX, true, NEED_G> &s, const R *v0, R &aw, R *av)
{
    opaque(s);
    R a0 = R(0), a1 = R(0), a2 = R(0);
    aw = R(0);
    IP_STENCIL_VALUE_GRADIENT(s, v0, aw, a0, a1, a2);
    av[0] = a0; av[1] = a1; av[2] = a2;
}

// ---- the finish of a loss held as one double per workgroup ------------------------------------------------------------------
constexpr int FINISH_WAYS = 8;

// slots (B, nslots) doubles -> loss (B) = scale * sum, in R.  One workgroup per batch item sums the item's slots in a fixed order.
// scale: 0.5 (ssd.hip) or -1 (lcc.hip); either product is exact in double.
template <typename R>
__global__ __launch_bounds__(BLOCK) void slot_finish(const double *__restrict__ slots, R *__restrict__ loss, int64_t nslots, int B, double scale)
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
        if (threadIdx.x == 0) loss[b] = (R)(scale * t);
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------
// Where the samples lie: o + disp[b, o, :] of a dense displacement field, or A_b o + t_b of one matrix per item.
// LATTICE_AFFINE_LOOPED: an affine lattice whose kernels all walk the batch in a loop (lcc_affine.hip), so the batch is not capped at
// the rows of a launch.
enum Lattice { LATTICE_FIELD, LATTICE_AFFINE, LATTICE_AFFINE_LOOPED };

// Validate + convert: vol_* is moving as interpol_pull takes its vol, grid_shape the sample lattice (LATTICE_FIELD: grid_* is disp),
// val_* is fixed as interpol_pull takes its val.  *mspan: the bytes one (batch, channel) image of moving spans.
static int problem_params(const interpol_problem *p, Lattice lat, KParams *k, int *B, uint64_t *mspan)
{
    const bool field = lat == LATTICE_FIELD;
    if (!p) return INTERPOL_E_NULL;
    if (p->abi_version != INTERPOL_ABI_VERSION) return INTERPOL_E_SHAPE;
    if (p->dim < 1 || p->dim > 3) return INTERPOL_E_DIM;
    if (p->extrapolate < 0 || p->extrapolate > 2) return INTERPOL_E_EXTRAP;
    if (p->dtype != INTERPOL_F32 && p->dtype != INTERPOL_F64) return INTERPOL_E_DTYPE;
    if (p->grid_dtype != p->dtype) return INTERPOL_E_DTYPE;
    // the batch: the kernels of a field loop over gridDim.y; those of an affine lattice have the item ON gridDim.y (LATTICE_AFFINE)
    if (p->batch < 1 || p->batch > (lat == LATTICE_AFFINE ? 65535 : 0x7fffffff) || p->channels < 1 || p->channels > 0x7fffffff) return INTERPOL_E_SHAPE;
    // the lattice is what the entry point says it is: a dense field is neither separable nor affine, a matrix holds no displacements
    if (p->flags & (INTERPOL_FLAG_SEPARABLE_GRID | (field ? INTERPOL_FLAG_AFFINE_GRID : INTERPOL_FLAG_DISPLACEMENT))) return INTERPOL_E_STRIDE;
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
    // fixed, and the displacements of a field (point by point): row-major over the sample lattice; a matrix has no grid strides to check
    if (field && D > 1 && p->grid_stride[4] != 1) return INTERPOL_E_STRIDE;
    int64_t gexp = D, fexp = 1, N = 1;
    for (int d = D - 1; d >= 0; --d) {
        if (p->grid_shape[d] > 1 && ((field && p->grid_stride[1 + d] != gexp) || p->val_stride[2 + d] != fexp)) return INTERPOL_E_STRIDE;
        gexp *= p->grid_shape[d];
        fexp *= p->grid_shape[d];
        N *= p->grid_shape[d];
        if (N > 0xffffffffll) return INTERPOL_E_SHAPE;              // the sample index is split in 32 bits (load_coords)
    }
    if (p->vol_stride[0] < 0 || p->vol_stride[1] < 0 || (field && p->grid_stride[0] < 0) || p->val_stride[0] < 0 || p->val_stride[1] < 0)
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
    // load_coords: 2 = `disp` holds displacements, the lattice is added; 3 = x = A o + t from the matrix
    k->sep = field ? 2 : 3;
    k->N = N;
    k->vol_sb = p->vol_stride[0];
    k->vol_sc = p->vol_stride[1];
    k->grid_sb = field ? p->grid_stride[0] : 0;                     // (a matrix comes with a batch stride of its own)
    k->val_sb = p->val_stride[0];
    k->val_sc = p->val_stride[1];
    *B = (int)p->batch;
    return 0;
}

// the bytes a call reads of moving (mimage: *mspan of problem_params), of fixed and of a weight (B, *shape) with its batch stride
static uint64_t moving_bytes(const KParams &k, uint64_t B, uint64_t es, uint64_t mimage)
{
    return ((B - 1) * (uint64_t)k.vol_sb + ((uint64_t)k.C - 1) * (uint64_t)k.vol_sc) * es + mimage;
}
static uint64_t fixed_bytes(const KParams &k, uint64_t B, uint64_t es)
{
    return ((B - 1) * (uint64_t)k.val_sb + ((uint64_t)k.C - 1) * (uint64_t)k.val_sc + (uint64_t)k.N) * es;
}
static uint64_t weight_bytes(const KParams &k, uint64_t B, uint64_t es, const void *weight, int64_t weight_batch_stride)
{
    return weight ? ((B - 1) * (uint64_t)weight_batch_stride + (uint64_t)k.N) * es : 0;
}

// What is written overlaps neither what is read nor anything else that is written.  0 bytes: absent.
struct Range { const void *ptr; uint64_t bytes; };
static int ranges_alias(const Range *rd, int nr, const Range *wr, int nw)
{
    for (int i = 0; i < nw; ++i) {
        if (!wr[i].bytes) continue;
        for (int j = 0; j < nr; ++j)
            if (rd[j].bytes && reg::ranges_overlap(wr[i].ptr, wr[i].bytes, rd[j].ptr, rd[j].bytes)) return INTERPOL_E_STRIDE;
        for (int j = i + 1; j < nw; ++j)
            if (wr[j].bytes && reg::ranges_overlap(wr[i].ptr, wr[i].bytes, wr[j].ptr, wr[j].bytes)) return INTERPOL_E_STRIDE;
    }
    return 0;
}

// f(R(), integral_constant<int, D>(), integral_constant<int, KMAX>()) for the dtype (float / double), dim 1..3 and order 1..3 of a
// validated problem: what remains a run-time choice (the Hessian kind, the ring) is the data term's own.
template <typename R, int D, typename F>
static void dispatch_order(int order, const F &f)
{
    switch (order) {
    case 1: return f(R(), std::integral_constant<int, D>(), std::integral_constant<int, 1>());
    case 2: return f(R(), std::integral_constant<int, D>(), std::integral_constant<int, 2>());
    default: return f(R(), std::integral_constant<int, D>(), std::integral_constant<int, 3>());
    }
}
template <typename R, typename F>
static void dispatch_dim(const KParams &k, const F &f)
{
    switch (k.dim) {
    case 1: return dispatch_order<R, 1>(k.order[0], f);
    case 2: return dispatch_order<R, 2>(k.order[0], f);
    default: return dispatch_order<R, 3>(k.order[0], f);
    }
}
template <typename F>
static void dispatch(const interpol_problem *p, const KParams &k, const F &f)
{
    if (p->dtype == INTERPOL_F64) dispatch_dim<double>(k, f);
    else dispatch_dim<float>(k, f);
}

} // namespace dt
} // namespace ip
