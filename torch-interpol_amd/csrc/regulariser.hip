// ===========================================================================
// regulariser.hip -- the smoothness penalty of a voxel displacement field v (B, *shape, D): absolute, membrane, bending.
//
//     (L v)_d = h_d^2 [ absolute v_d + membrane sum_e A_e v_d + bending ( sum_e B_e v_d + sum_{e != f} A_e A_f v_d ) ]
//     A_e f [o] = (2 f~[o] - f~[o - e] - f~[o + e]) / h_e^2
//     B_e f [o] = (f~[o - 2e] - 4 f~[o - e] + 6 f~[o] - 4 f~[o + e] + f~[o + 2e]) / h_e^4
//
// f~[i] = wrap_sign(i) f[wrap_index(i)] along the axis of the stencil, for EVERY tap of A_e / B_e, the centre included
// (spline_math.hpp; dst1 keeps its quirk: the sign is 0 at index 0).  A_e A_f is the tensor product of the two 1-D stencils.
// In 3-D with bending that is 25 points: the centre, 6 + 6 along the axes and 12 in-plane diagonals (unit voxels, bending = 1:
// centre 42, |coefficients| sum to 144).
//
//   reg_fwd<R, D, MODE>    : one thread = one lattice point, in storage order (the organisation of jacobian.hip); per tap ONE
//                            D-component load; writes L v in the layout of the field.
//   reg_energy<R, D, MODE> : RG_BLOCKS persistent workgroups per batch item, each over a run of consecutive points; every thread forms
//                            v_d (L v)_d in DOUBLE whatever R is (reg_at<R, D, MODE, double>, the coefficient tables unrounded) and keeps
//                            its sum in double: where the field is smooth, or nearly constant under a bound that has the constants in the
//                            null space of L, the taps cancel, and the rounding of float32 products is then large against the energy
//                            itself (55 times the 1e-5 bar on a nearly constant line of four points); block_sum1, one double per workgroup into the
//                            workspace (every workgroup writes its row: the workspace need not be cleared);
//   reg_energy_finish<R>   : one workgroup per batch item sums its RG_BLOCKS rows the same way and writes 0.5 * sum.
//                            No atomics, and the summation tree of an item depends neither on the shape nor on the batch:
//                            bit-identical from run to run, and for an item alone or inside a batch (the scheme of affine_grad.hip).
//
// The linear-elastic terms (interpol_regulariser_elastic; weights shears, div), coupling the components:
//     (L v)_c += h_c^2 [ shears sum_e A_e v_c + (shears + div) A_c v_c ]  -  (shears + div) sum_{e != c} X_ce v_e
//     X_ce f [o] = ( f~[o + c + e] - f~[o + c - e] - f~[o - c + e] + f~[o - c - e] ) / 4
// shears folds into the membrane weights, the own-axis extra into a second table for component c along c, and X_ce lives on
// the in-plane diagonals that the mixed bending terms load: 25 points with bending, 7 + 12 = 19 without.  In a SLIDING
// dimension d the kernels index as dct2 and component d takes the signs of dst2 along d (the same index map): the flips are
// found behind the inside test, next to the wrapped indices, and folded into the per-component tables.
//
// MODE: bit 0 absolute, bit 1 membrane, bit 2 bending, bit 3 elastic and / or sliding (always with bit 1) -- the terms that are present.  A term whose weight is zero costs
// nothing: membrane alone loads 2 D + 1 points, absolute alone the centre only, and the per-axis coefficient tables are
// combined on the host.  11 modes (1..7, 10, 11, 14, 15) x D = 1..3 x float / double; the first seven are the code they were.
//
// Per axis the indices and signs of the taps are wrap_index / wrap_sign behind one inside test (as jac_at); signs are folded
// into the per-axis weights, (v * s) * w == v * (s * w) exactly for s in {-1, 0, 1}.
//
// Every thread gathers from the field, so the output must not overlap it (validated by the entry point).
// The C entry points live here as well (include/interpol_hip.h: interpol_regulariser, interpol_regulariser_energy).
// ===========================================================================
#include "regulariser_at.hpp"                                      // PointVec, Weights, reg_at, block_sum1, reg_params, reg_weights, ...

namespace ip {
namespace reg {

// field (B, *shape, D) through p.vol_sb / p.vol_ss (bytes); out (B, *shape, D) dense per item through p.val_sb
template <typename R, int D, int MODE>
__global__ __launch_bounds__(BLOCK) void reg_fwd(KParams p, WeightsOf<R, MODE> w, const R *__restrict__ field, R *__restrict__ out, int B)
{
    typedef PointVec<R, D> V;
    const int64_t o = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (o >= p.N) return;
    unsigned od[3];
    split_index<D>(p, o, od);
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        V v0, r;
        reg_at<R, D, MODE>(p, w, reinterpret_cast<const V *>(field + b * p.vol_sb), od, v0, r.c);
        *reinterpret_cast<V *>(out + b * p.val_sb + o * D) = r;
    }
}

// rows (B, RG_BLOCKS) doubles: rows[b][g] = the sum of v . L v over the points of item b that workgroup g visits
template <typename R, int D, int MODE>
__global__ __launch_bounds__(BLOCK) void reg_energy(KParams p, WeightsOf<double, MODE> w, const R *__restrict__ field, double *__restrict__ rows, int B)
{
    typedef PointVec<R, D> V;
    __shared__ double part[BLOCK / 64];
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        const V *ub = reinterpret_cast<const V *>(field + b * p.vol_sb);
        double acc = 0.0;
        // a workgroup owns a run of consecutive points (whole multiples of BLOCK): its rows and planes stay in L1 / L2
        const int64_t chunk = ((p.N + RG_BLOCKS - 1) / RG_BLOCKS + BLOCK - 1) / BLOCK * BLOCK;
        const int64_t lo = blockIdx.x * chunk, hi = lo + chunk < p.N ? lo + chunk : p.N;
        for (int64_t o = lo + threadIdx.x; o < hi; o += BLOCK) {
            unsigned od[3];
            split_index<D>(p, o, od);
            V v0;
            double lv[D];
            reg_at<R, D, MODE, double>(p, w, ub, od, v0, lv);
#pragma unroll
            for (int c = 0; c < D; ++c) acc += (double)v0.c[c] * lv[c];
        }
        const double s = block_sum1(acc, part);
        if (threadIdx.x == 0) rows[b * RG_BLOCKS + blockIdx.x] = s;
    }
}

template <typename R>
__global__ __launch_bounds__(BLOCK) void reg_energy_finish(const double *__restrict__ rows, R *__restrict__ energy, int B)
{
    __shared__ double part[BLOCK / 64];
    for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
        double acc = 0.0;
        for (int r = threadIdx.x; r < RG_BLOCKS; r += BLOCK) acc += rows[b * RG_BLOCKS + r];
        const double s = block_sum1(acc, part);
        if (threadIdx.x == 0) energy[b] = (R)(0.5 * s);
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------
template <typename R, int D, int MODE>
static void reg_launch(bool energy, const KParams &k, const WeightsEL<double> &wd, const void *field, void *out, void *rows, int B, hipStream_t st)
{
    const WeightsOf<R, MODE> w = narrow<R>(wd);                       // (the three-term modes: the first part alone)
    const WeightsOf<double, MODE> we = wd;
    const unsigned by = (unsigned)(B < 65535 ? B : 65535);
    if (energy) {
        hipLaunchKernelGGL((reg_energy<R, D, MODE>), dim3(RG_BLOCKS, by, 1), dim3(BLOCK), 0, st, k, we, (const R *)field, (double *)rows, B);
        hipLaunchKernelGGL((reg_energy_finish<R>), dim3(by), dim3(BLOCK), 0, st, (const double *)rows, (R *)out, B);
    } else {
        const int64_t nb = (k.N + BLOCK - 1) / BLOCK;               // (< 2^22: N < 2^30)
        hipLaunchKernelGGL((reg_fwd<R, D, MODE>), dim3((unsigned)nb, by, 1), dim3(BLOCK), 0, st, k, w, (const R *)field, (R *)out, B);
    }
}

template <typename R, int D>
static void reg_by_mode(int mode, bool energy, const KParams &k, const WeightsEL<double> &w, const void *field, void *out, void *rows, int B, hipStream_t st)
{
    switch (mode) {
    case 1: return reg_launch<R, D, 1>(energy, k, w, field, out, rows, B, st);
    case 2: return reg_launch<R, D, 2>(energy, k, w, field, out, rows, B, st);
    case 3: return reg_launch<R, D, 3>(energy, k, w, field, out, rows, B, st);
    case 4: return reg_launch<R, D, 4>(energy, k, w, field, out, rows, B, st);
    case 5: return reg_launch<R, D, 5>(energy, k, w, field, out, rows, B, st);
    case 6: return reg_launch<R, D, 6>(energy, k, w, field, out, rows, B, st);
    case 7: return reg_launch<R, D, 7>(energy, k, w, field, out, rows, B, st);
    case 10: return reg_launch<R, D, 10>(energy, k, w, field, out, rows, B, st);
    case 11: return reg_launch<R, D, 11>(energy, k, w, field, out, rows, B, st);
    case 14: return reg_launch<R, D, 14>(energy, k, w, field, out, rows, B, st);
    default: return reg_launch<R, D, 15>(energy, k, w, field, out, rows, B, st);
    }
}

template <typename R>
static void reg_by_dim(int mode, bool energy, const KParams &k, const WeightsEL<double> &w, const void *field, void *out, void *rows, int B, hipStream_t st)
{
    switch (k.dim) {
    case 1: return reg_by_mode<R, 1>(mode, energy, k, w, field, out, rows, B, st);
    case 2: return reg_by_mode<R, 2>(mode, energy, k, w, field, out, rows, B, st);
    default: return reg_by_mode<R, 3>(mode, energy, k, w, field, out, rows, B, st);
    }
}

static int64_t energy_workspace_bytes(int64_t B) { return B * RG_BLOCKS * (int64_t)sizeof(double); }

// 0 or a negative INTERPOL_E_* (a failed launch: INTERPOL_E_LAUNCH).  wt: absolute, membrane, bending, shears, div;
// sliding: INTERPOL_BOUND_SLIDING is a bound (the elastic entry points)
static int reg_entry(const interpol_problem *p, bool energy, const void *field, void *out, const double *wt, bool sliding,
                     const double *voxel_size, void *workspace, int64_t workspace_bytes, void *stream)
{
    KParams k; int B, slide = 0;
    const int rc = reg_params(p, !energy, &k, &B, sliding ? &slide : nullptr);
    if (rc) return rc;
    if (!wt) return INTERPOL_E_NULL;
    WeightsEL<double> w;
    const int mode = reg_weights(k.dim, wt[0], wt[1], wt[2], wt[3], wt[4], slide, voxel_size, &w);
    if (mode < 0) return mode;
    if (!field || !out) return INTERPOL_E_NULL;
    const uint64_t es = p->dtype == INTERPOL_F64 ? 8 : 4;
    const uint64_t item = (uint64_t)k.N * k.dim * es;
    const uint64_t fspan = (uint64_t)(B - 1) * (uint64_t)k.vol_sb * es + item;
    if (energy) {
        if (!workspace) return INTERPOL_E_NULL;
        if (workspace_bytes < energy_workspace_bytes(B)) return INTERPOL_E_SCRATCH;
        if (ranges_overlap(field, fspan, out, (uint64_t)B * es) || ranges_overlap(field, fspan, workspace, (uint64_t)energy_workspace_bytes(B))
            || ranges_overlap(out, (uint64_t)B * es, workspace, (uint64_t)energy_workspace_bytes(B)))
            return INTERPOL_E_STRIDE;
    } else if (ranges_overlap(field, fspan, out, (uint64_t)(B - 1) * (uint64_t)k.val_sb * es + item)) {
        return INTERPOL_E_STRIDE;                                   // other lattice points gather from the field
    }
    hipStream_t st = (hipStream_t)stream;
    if (p->dtype == INTERPOL_F64) reg_by_dim<double>(mode, energy, k, w, field, out, workspace, B, st);
    else reg_by_dim<float>(mode, energy, k, w, field, out, workspace, B, st);
    return hipGetLastError() == hipSuccess ? 0 : INTERPOL_E_LAUNCH;
}

} // namespace reg
} // namespace ip

extern "C" {

int interpol_regulariser(const interpol_problem *p, const void *field, void *out, double absolute, double membrane, double bending,
                         const double *voxel_size, void *stream)
{
    const double wt[5] = { absolute, membrane, bending, 0.0, 0.0 };
    return ip::reg::reg_entry(p, false, field, out, wt, false, voxel_size, nullptr, 0, stream);
}

int64_t interpol_regulariser_energy_workspace(const interpol_problem *p)
{
    ip::KParams k; int B;
    const int rc = ip::reg::reg_params(p, false, &k, &B);
    return rc ? rc : ip::reg::energy_workspace_bytes(B);
}

int interpol_regulariser_energy(const interpol_problem *p, const void *field, void *energy, double absolute, double membrane, double bending,
                                const double *voxel_size, void *workspace, int64_t workspace_bytes, void *stream)
{
    const double wt[5] = { absolute, membrane, bending, 0.0, 0.0 };
    return ip::reg::reg_entry(p, true, field, energy, wt, false, voxel_size, workspace, workspace_bytes, stream);
}

int interpol_regulariser_elastic(const interpol_problem *p, const void *field, void *out, const double *weights, const double *voxel_size,
                                 void *stream)
{
    return ip::reg::reg_entry(p, false, field, out, weights, true, voxel_size, nullptr, 0, stream);
}

int64_t interpol_regulariser_elastic_energy_workspace(const interpol_problem *p)
{
    ip::KParams k; int B, slide;
    const int rc = ip::reg::reg_params(p, false, &k, &B, &slide);
    return rc ? rc : ip::reg::energy_workspace_bytes(B);
}

int interpol_regulariser_elastic_energy(const interpol_problem *p, const void *field, void *energy, const double *weights,
                                        const double *voxel_size, void *workspace, int64_t workspace_bytes, void *stream)
{
    return ip::reg::reg_entry(p, true, field, energy, weights, true, voxel_size, workspace, workspace_bytes, stream);
}

} // extern "C"

#ifdef IP_EXPERIMENTS
#include "../experiments/regulariser_tile.inc"                       // the LDS halo tile, measured slower (interpol_regulariser_tile)
#endif
