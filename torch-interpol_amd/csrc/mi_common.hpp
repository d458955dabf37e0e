// ===========================================================================
// mi_common.hpp -- what the two mutual-information data terms share (mi_affine.hip on the matrix of an affine lattice, mi.hip on a
// dense displacement field): everything between the sample (I, J, omega) and the per-sample terms that does not care what kind
// of lattice the samples lie on.
//
//   MIN_BINS, MAX_BINS, RANGE_STRIDE, MI_BLOCKS : the bin constants, the doubles per item of `ranges`, the persistent workgroups
//                              of a histogram stage per item
//   quantum_shift            : the shift of the quantum q = wmax 2^-shift of the fixed-point histogram
//   Bins<R>, sample_bins<R>  : the tap base, the fixed bin, f = u - floor(u) and the clamp flag of a sample
//   bspline3, bspline3_d1, bspline3_abs_d2 : the cubic B-spline at the four taps, its first and its absolute second derivative
//   mi_clear<U>              : the kernel that clears the histogram region of the workspace
//   mi_table<R>              : the kernel that turns an item's histogram into T, 1 / W, the loss and P
//   stage_table<R>           : T of an item into dynamic LDS
//   hist_bytes, invw_bytes   : the head of both workspaces
//
// The two kernels are templates (mi_clear on the integer type, for that reason alone): each of the two files instantiates its own
// copy under one name, as dt::slot_finish is shared by ssd.hip and lcc.hip.  The per-sample bodies of the histogram stage and of
// the third stage stay in their files: mi_affine.hip's kernels are instruction for instruction what they were (profiles/mi.txt).
// ===========================================================================
#pragma once
#include "data_term.hpp"

namespace ip {
namespace mi {

using namespace dt;

// Persistent workgroups of a histogram stage per batch item.  The histogram does not depend on it (integer sums).
constexpr int MI_BLOCKS = 512;
constexpr int MIN_BINS = 8, MAX_BINS = 64;
constexpr int RANGE_STRIDE = 5;                                     // doubles per item: m_lo, m_sc, f_lo, f_sc, wmax

// shift of the quantum q = wmax 2^-shift: min(52, 62 - ceil(log2 N))
static int quantum_shift(int64_t N)
{
    int lg = 0;
    while (((int64_t)1 << lg) < N) ++lg;
    return 62 - lg < 52 ? 62 - lg : 52;
}

// What a sample contributes to: the tap base j0 = floor(u) - 1 on the moving side and the bin k on the fixed side; f = u - floor(u);
// clamped: t_m left [0, 1].
template <typename R>
struct Bins { int j0, k; R f; bool clamped; };

template <typename R>
__device__ __forceinline__ Bins<R> sample_bins(R I, R J, R m_lo, R m_sc, R f_lo, R f_sc, int B)
{
    Bins<R> r;
    const R raw = (I - m_lo) * m_sc;
    r.clamped = !(raw >= R(0) && raw <= R(1));
    const R tm = raw < R(0) ? R(0) : (raw > R(1) ? R(1) : raw);
    const R u = fma_(tm == tm ? tm : R(0), (R)(B - 4), R(1.5));
    int fl = (int)floor(u);
    fl = fl < 1 ? 1 : (fl > B - 3 ? B - 3 : fl);
    r.f = u - (R)fl;
    r.j0 = fl - 1;
    const R rf = (J - f_lo) * f_sc;
    const R tf = rf < R(0) ? R(0) : (rf > R(1) ? R(1) : rf);
    int k = (int)floor(fma_(tf == tf ? tf : R(0), (R)(B - 1), R(0.5)));
    r.k = k < 0 ? 0 : (k > B - 1 ? B - 1 : k);
    return r;
}

// the cubic B-spline at the four taps, f in [0, 1): weights, first and second derivative with respect to u
template <typename R>
__device__ __forceinline__ void bspline3(R f, R *w)
{
    const R g = R(1) - f;
    w[0] = g * g * g * R(1.0 / 6.0);
    w[1] = R(2.0 / 3.0) - f * f + R(0.5) * f * f * f;
    w[2] = R(2.0 / 3.0) - g * g + R(0.5) * g * g * g;
    w[3] = f * f * f * R(1.0 / 6.0);
}
template <typename R>
__device__ __forceinline__ void bspline3_d1(R f, R *w)
{
    const R g = R(1) - f;
    w[0] = R(-0.5) * g * g;
    w[1] = R(-2) * f + R(1.5) * f * f;
    w[2] = R(2) * g - R(1.5) * g * g;
    w[3] = R(0.5) * f * f;
}
template <typename R>
__device__ __forceinline__ void bspline3_abs_d2(R f, R *w)
{
    w[0] = R(1) - f;
    w[1] = fabs(R(3) * f - R(2));
    w[2] = fabs(R(1) - R(3) * f);
    w[3] = f;
}

// ---- stage 1: the joint histogram in 64-bit fixed point ----------------------------------------------------------------
template <typename U>
__global__ __launch_bounds__(BLOCK) void mi_clear(U *__restrict__ hist, int64_t count)
{
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < count; i += (int64_t)gridDim.x * BLOCK) hist[i] = 0ull;
}

// ---- stage 2: P, the marginals, T and the loss ------------------------------------------------------------------------
template <typename R>
__global__ __launch_bounds__(BLOCK) void mi_table(const long long *__restrict__ hist, const double *__restrict__ ranges,
                                                  R *__restrict__ table, double *__restrict__ inv_w, R *__restrict__ loss,
                                                  R *__restrict__ histogram, int bins, int shift)
{
    __shared__ long long h[MAX_BINS * MAX_BINS];
    __shared__ long long row[MAX_BINS], col[MAX_BINS];
    __shared__ long long total;
    __shared__ double part[BLOCK];
    const int64_t b = blockIdx.x;
    const int nb = bins * bins;
    const long long *hb = hist + b * nb;
    for (int i = threadIdx.x; i < nb; i += BLOCK) h[i] = hb[i];
    __syncthreads();
    if ((int)threadIdx.x < bins) {
        long long t = 0;
        for (int k = 0; k < bins; ++k) t += h[threadIdx.x * bins + k];
        row[threadIdx.x] = t;
    } else if ((int)threadIdx.x < 2 * bins) {
        const int k = threadIdx.x - bins;
        long long t = 0;
        for (int j = 0; j < bins; ++j) t += h[j * bins + k];
        col[k] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        long long t = 0;
        for (int j = 0; j < bins; ++j) t += row[j];
        total = t;
    }
    __syncthreads();
    const long long tot = total;
    const double wmax = ranges[b * RANGE_STRIDE + 4];
    const bool live = tot > 0 && wmax > 0.0;
    const double inv_tot = live ? 1.0 / (double)tot : 0.0;
    double acc = 0.0;
    for (int i = threadIdx.x; i < nb; i += BLOCK) {
        const int j = i / bins, k = i - j * bins;
        const long long v = h[i];
        double P = 0.0, T = 0.0;
        if (live) {
            P = (double)v * inv_tot;
            if (v > 0) {
                T = log(P / (((double)row[j] * inv_tot) * ((double)col[k] * inv_tot)));
                acc = __builtin_fma(P, T, acc);
            }
        }
        table[b * nb + i] = (R)T;
        if (histogram) histogram[b * nb + i] = (R)P;
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int off = BLOCK / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        loss[b] = (R)(-part[0]);
        inv_w[b] = live ? 1.0 / ((double)tot * ldexp(wmax, -shift)) : 0.0;     // W = total q
    }
}

// ---- stage 3: T in LDS ------------------------------------------------------------------------------------------------
template <typename R>
__device__ __forceinline__ R *stage_table(const R *__restrict__ table, int64_t b, int bins)
{
    extern __shared__ double lds_table[];                           // bins x bins of R (declared double: 8-byte aligned for both)
    R *T = (R *)lds_table;
    const int nb = bins * bins;
    for (int i = threadIdx.x; i < nb; i += BLOCK) T[i] = table[b * nb + i];
    __syncthreads();
    return T;
}

// the workspace both terms begin with: the integer histograms, T (8 bytes per entry reserved), 1 / W
static int64_t hist_bytes(int B, int bins) { return (int64_t)B * bins * bins * 8; }
static int64_t invw_bytes(int B) { return (int64_t)B * 8; }

} // namespace mi
} // namespace ip
