// ===========================================================================
// lcc_common.hpp -- what the local cross-correlation data terms share (lcc.hip on a dense displacement field, lcc_affine.hip on
// the matrix of an affine lattice): the tile of a workgroup and the lattice taken as three dims (Win), the window sum
// (window_march), the statistics stage (Stats, lcc_stats: the five window sums down to a, c, f and the loss), the tiling and the
// workspace helpers.  lcc.hip describes the stages; what every data term shares lives in data_term.hpp.
// ===========================================================================
#pragma once
#include "data_term.hpp"
#include "point_field.hpp"                                         // compose_sample, compose_blocks

namespace ip {
namespace lcc {

using namespace dt;

constexpr int TY = 8, TZ = 32, XC = 32;                            // the tile of a workgroup (TY * TZ == BLOCK) and its chunk along x
constexpr int RMAX = 4;                                            // window <= 9
constexpr int HY = TY + 2 * RMAX, HZ = TZ + 2 * RMAX;              // the halo'd tile
static_assert(TY * TZ == BLOCK, "one column per thread");

// the lattice as three dims (leading extents 1, radii 0), and how the workgroups tile it
struct Win { int n[3]; int r[3]; int ty, tz, cx; };
struct Strides { int64_t weight, gradient, hessian; };             // (a kernel parameter: its namespace is part of the kernels' names)

// ---- the window sum ----------------------------------------------------------------------------------------------------------
// P: NQ fields of T go in, NS double sums come out.  P::load(q, lin), P::accumulate(v, s) (one point into the sums), P::merge(s, part)
// (partial sums into the sums), P::epilogue(lin, n, s).
template <typename T, int NQ, int NS, int WX, typename P>
__device__ __forceinline__ void window_march(const Win &w, P &pol, T (*raw)[HY][HZ], double (*tmp)[HY][TZ], double (*ring)[NS][BLOCK])
{
    unsigned bi = blockIdx.x;
    const int bz = (int)(bi % (unsigned)w.tz); bi /= (unsigned)w.tz;
    const int by = (int)(bi % (unsigned)w.ty), bx = (int)(bi / (unsigned)w.ty);
    const int x0 = bx * XC, y0 = by * TY, z0 = bz * TZ;
    const int x1 = min(x0 + XC, w.n[0]);                            // this workgroup's output planes: [x0, x1)
    const int rx = w.r[0], ry = w.r[1], rz = w.r[2];
    const int hy = TY + 2 * ry, hz = TZ + 2 * rz;
    const int tid = threadIdx.x, ly = tid / TZ, lz = tid % TZ;
    const int y = y0 + ly, z = z0 + lz;
    const bool mine = y < w.n[1] && z < w.n[2];
    const int ny = min(y + ry, w.n[1] - 1) - max(y - ry, 0) + 1, nz = min(z + rz, w.n[2] - 1) - max(z - rz, 0) + 1;
    const int lo = max(x0 - rx, 0), hi = min(x1 - 1 + rx, w.n[0] - 1);
    for (int xp = lo; xp <= hi; ++xp) {
        // 1. the plane's halo'd tile; zeros outside the lattice
        for (int i = tid; i < hy * hz; i += BLOCK) {
            const int yy = i / hz, zz = i - yy * hz;
            const int gy = y0 - ry + yy, gz = z0 - rz + zz;
            const bool in = gy >= 0 && gy < w.n[1] && gz >= 0 && gz < w.n[2];
            const int64_t lin = ((int64_t)xp * w.n[1] + gy) * w.n[2] + gz;
#pragma unroll
            for (int q = 0; q < NQ; ++q) raw[q][yy][zz] = in ? pol.load(q, lin) : T(0);
        }
        __syncthreads();
        // 2. along z, ascending
        for (int i = tid; i < hy * TZ; i += BLOCK) {
            const int yy = i / TZ, zz = i % TZ;
            double s[NS];
#pragma unroll
            for (int k = 0; k < NS; ++k) s[k] = 0.0;
            for (int t = 0; t <= 2 * rz; ++t) {
                T v[NQ];
#pragma unroll
                for (int q = 0; q < NQ; ++q) v[q] = raw[q][yy][zz + t];
                P::accumulate(v, s);
            }
#pragma unroll
            for (int k = 0; k < NS; ++k) tmp[k][yy][zz] = s[k];
        }
        __syncthreads();
        // 3. along y, ascending, into this thread's column of the ring
        {
            double s[NS];
#pragma unroll
            for (int k = 0; k < NS; ++k) s[k] = 0.0;
            for (int t = 0; t <= 2 * ry; ++t) {
                double part[NS];
#pragma unroll
                for (int k = 0; k < NS; ++k) part[k] = tmp[k][ly + t][lz];
                P::merge(s, part);
            }
#pragma unroll
            for (int k = 0; k < NS; ++k) ring[xp % WX][k][tid] = s[k];
        }
        // 4. the output planes whose window ends at this input plane: xo = xp - rx, and at the lattice's last plane all that are left
        if (mine) {
            const int first = max(xp - rx, x0), last = xp == w.n[0] - 1 ? x1 - 1 : min(xp - rx, x1 - 1);
            for (int xo = first; xo <= last; ++xo) {
                const int plo = max(xo - rx, 0), phi = min(xo + rx, w.n[0] - 1);
                double s[NS];
#pragma unroll
                for (int k = 0; k < NS; ++k) s[k] = 0.0;
                for (int pl = plo; pl <= phi; ++pl) {
                    double part[NS];
#pragma unroll
                    for (int k = 0; k < NS; ++k) part[k] = ring[pl % WX][k][tid];
                    P::merge(s, part);
                }
                pol.epilogue(((int64_t)xo * w.n[1] + y) * w.n[2] + z, (phi - plo + 1) * ny * nz, s);
            }
        }
        // (the next plane's step 1 writes `raw`, which nobody reads after the barrier of step 2; its barrier orders step 3 before
        //  the next step 2 writes `tmp`)
    }
    __syncthreads();
}

// ---- stage 2: the statistics ------------------------------------------------------------------------------------------------------
// COMP: every one of the five sums carries the rounding errors of its additions (and of its products) in a second double: sums [0, 5)
// are the sums, [5, 10) their error terms, and the central moments are formed from the pairs.  S_II - S_I^2 / n cancels: with three
// nearly equal points in a window the plain double sums leave 4e-16 / vI in vI, which a den that falls to eps = 1e-5 turns into 1e-11
// of the gradient -- the whole float64 bar.  From float32 images the products are exact in double and the sums nearly so: R = float
// needs none of it.  (R = double with a ring of nine planes has no LDS left for the second set and sums plainly.)
// (no contraction in these: a product fused into the sum that TwoSum takes apart would not be the product whose error is carried)
__device__ __forceinline__ void add_pair(double *s, int k, double x, double xlo)
{
#pragma clang fp contract(off)
    const double t = s[k] + x, bb = t - s[k];
    const double err = (s[k] - (t - bb)) + (x - bb);                // TwoSum: s[k] + x == t + err exactly
    s[k] = t;
    s[5 + k] += err + xlo;
}
// (n S_XY - S_X S_Y) / n from the pairs
__device__ __forceinline__ double central(double n, double xy, double xylo, double x, double xlo, double y, double ylo)
{
#pragma clang fp contract(off)
    const double p1 = n * xy, e1 = fma_(n, xy, -p1);
    const double p2 = x * y, e2 = fma_(x, y, -p2);
    const double d = p1 - p2, bb = d - p1;
    const double de = (p1 - (d - bb)) + (-p2 - bb);
    return (d + (de + (e1 - e2) + n * xylo - (x * ylo + xlo * y))) / n;
}

template <typename R, bool COMP> struct Stats {
    static constexpr int NS = COMP ? 10 : 5;
    const R *I, *J, *weight; double *acf; int64_t N; double eps, loss;
    __device__ __forceinline__ R load(int q, int64_t lin) const { return q == 0 ? I[lin] : J[lin]; }
    static __device__ __forceinline__ void accumulate(const R *v, double *s)
    {
        const double i = (double)v[0], j = (double)v[1];
        if (COMP) {
#pragma clang fp contract(off)
            const double ii = i * i, jj = j * j, ij = i * j;
            add_pair(s, 0, i, 0.0); add_pair(s, 1, j, 0.0);
            add_pair(s, 2, ii, fma_(i, i, -ii)); add_pair(s, 3, jj, fma_(j, j, -jj)); add_pair(s, 4, ij, fma_(i, j, -ij));
        } else {
            s[0] += i; s[1] += j; s[2] += i * i; s[3] += j * j; s[4] += i * j;
        }
    }
    static __device__ __forceinline__ void merge(double *s, const double *part)
    {
        if (COMP) {
#pragma unroll
            for (int k = 0; k < 5; ++k) add_pair(s, k, part[k], part[5 + k]);
        } else {
#pragma unroll
            for (int k = 0; k < 5; ++k) s[k] += part[k];
        }
    }
    __device__ __forceinline__ void epilogue(int64_t lin, int count, const double *s)
    {
        const double n = (double)count;
        double cross, vI, vJ, SI = s[0], SJ = s[1];
        if (COMP) {
            cross = central(n, s[4], s[9], s[0], s[5], s[1], s[6]);
            vI = fmax(central(n, s[2], s[7], s[0], s[5], s[0], s[5]), 0.0);
            vJ = fmax(central(n, s[3], s[8], s[1], s[6], s[1], s[6]), 0.0);
            SI += s[5]; SJ += s[6];
        } else {
            cross = s[4] - s[0] * s[1] / n;
            vI = fmax(s[2] - s[0] * s[0] / n, 0.0);
            vJ = fmax(s[3] - s[1] * s[1] / n, 0.0);
        }
        const double den = vI * vJ + eps;
        const double wt = weight ? (double)weight[lin] : 1.0;
        const double a = wt * 2.0 * cross / den, c = wt * 2.0 * cross * cross * vJ / (den * den);
        const double f = (a * SJ - c * SI) / n;
        acf[lin] = a; acf[N + lin] = c; acf[2 * N + lin] = f;
        loss += wt * (cross * cross / den);
    }
};

// I (B, C, N), fixed through p.val_sb / p.val_sc, acf (B, C, 3, N), slots (B, gridDim.x) doubles
template <typename R, int WX>
__global__ __launch_bounds__(BLOCK) void lcc_stats(KParams p, Win w, const R *__restrict__ I, const R *__restrict__ fixed,
                                                   const R *__restrict__ weight, double *__restrict__ acf, double *__restrict__ slots,
                                                   double eps, Strides sb, int B)
{
    constexpr bool COMP = sizeof(R) == sizeof(double) && WX <= 5;  // (the pairs of a ring of nine planes do not fit the LDS)
    typedef Stats<R, COMP> S;
    __shared__ R raw[2][HY][HZ];
    __shared__ double tmp[S::NS][HY][TZ];
    __shared__ double ring[WX][S::NS][BLOCK];
    __shared__ double part[BLOCK / 64];
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        S st;
        st.weight = weight ? weight + b * sb.weight : nullptr;
        st.N = p.N; st.eps = eps; st.loss = 0.0;
        for (int c = 0; c < p.C; ++c) {
            st.I = I + (b * p.C + c) * p.N;
            st.J = fixed + b * p.val_sb + c * p.val_sc;
            st.acf = acf + (b * p.C + c) * 3 * p.N;
            window_march<R, 2, S::NS, WX>(w, st, raw, tmp, ring);
        }
        const double t = reg::block_sum1(st.loss, part);
        if (threadIdx.x == 0) slots[b * gridDim.x + blockIdx.x] = t;
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------
// the lattice as three dims and its tiling; the radii are filled in by lcc_window
static Win lcc_tiling(const KParams &k)
{
    Win w;
    for (int d = 0; d < 3; ++d) { w.n[d] = 1; w.r[d] = 0; }
    for (int d = 0; d < k.dim; ++d) w.n[3 - k.dim + d] = k.gshape[d];
    w.cx = (w.n[0] + XC - 1) / XC;
    w.ty = (w.n[1] + TY - 1) / TY;
    w.tz = (w.n[2] + TZ - 1) / TZ;
    return w;
}
static int64_t lcc_groups(const Win &w) { return (int64_t)w.cx * w.ty * w.tz; }

static int64_t pull_blocks(const KParams &k)
{
    switch (k.dim) {
    case 1: return compose_blocks<1>(k);
    case 2: return compose_blocks<2>(k);
    default: return compose_blocks<3>(k);
    }
}

// the workspace: the slots (B, groups) and a, c, f (B, C, 3, N), doubles, then I (B, C, N) of the dtype
static uint64_t lcc_slot_bytes(uint64_t B, int64_t groups) { return B * (uint64_t)groups * sizeof(double); }
static uint64_t lcc_acf_bytes(const KParams &k, uint64_t B) { return 3 * B * (uint64_t)k.C * (uint64_t)k.N * sizeof(double); }
static uint64_t lcc_ws_bytes(const KParams &k, uint64_t B, int64_t groups, uint64_t es)
{
    const uint64_t image = B * (uint64_t)k.C * (uint64_t)k.N * es;
    return lcc_slot_bytes(B, groups) + lcc_acf_bytes(k, B) + ((image + 7) & ~(uint64_t)7);
}

} // namespace lcc
} // namespace ip
