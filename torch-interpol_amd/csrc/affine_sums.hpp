// ===========================================================================
// affine_sums.hpp -- what the data terms on the matrix of an AFFINE lattice share (ssd_affine.hip, mi_affine.hip, lcc_affine.hip): the value and
// the gradient of one stencil, the NS sums of a Gauss-Newton step held in double, their two organisations, the fixed-order
// reduction and the finish.  What every data term shares -- the validation of the problem (problem_params, LATTICE_AFFINE), the alias
// check, pair_index, stencil_value_gradient and the dispatch -- lives in data_term.hpp.  A data term supplies its per-sample terms as a functor
//
//     terms(o, od, lt, q, h):   od = (o_0 .. o_{D-1}, 1) as doubles,  lt the loss term,  q[d],  h[pair(d, d')] (HESS), formed in R
//
// and the sums are
//     [0]                                    lt
//     [1 + d (D+1) + e]                      q_d o~_e
//     [1 + P + pair(d,d') M + pair(e,e')]    h_dd' o~_e o~_e',   M = (D+1)(D+2)/2 moments, pair: upper triangle row by row
// NS = 1 + P + D(D+1)/2 * M: 73 / 25 / 6 for D = 3 / 2 / 1; without a Hessian 1 + P.  (o~_e o~_e' is exact in double whenever it is
// below 2^53.)  No atomics, nothing in the workspace is assumed cleared: the summation tree depends on the shape alone.
// ===========================================================================
#pragma once
#include "data_term.hpp"

namespace ip {
namespace ssd_affine {

using namespace dt;

// Persistent workgroups of the partial sums per batch item = doubles per sum and item in the workspace.  A CONSTANT.
constexpr int SA_BLOCKS = 1024;
constexpr int WAVES = BLOCK / 64;
constexpr int FINISH_WAYS = SA_BLOCKS / 64;                         // the doubles of one sum that one lane of the finish adds

constexpr int params(int D) { return D * (D + 1); }
constexpr int moments(int D) { return (D + 1) * (D + 2) / 2; }
constexpr int num_sums(int D, bool hess) { return 1 + params(D) + (hess ? (D * (D + 1) / 2) * moments(D) : 0); }

// od = (o_0 .. o_{D-1}, 1) as doubles (the split of load_coords)
template <int D>
__device__ __forceinline__ void sample_index(const KParams &p, int64_t o, double *od)
{
    unsigned rr = (unsigned)o;
#pragma unroll
    for (int d = D - 1; d > 0; --d) { const unsigned qq = rr / (unsigned)p.gshape[d]; od[d] = (double)(rr - qq * (unsigned)p.gshape[d]); rr = qq; }
    od[0] = (double)rr;
    od[D] = 1.0;
}

// SA_BLOCKS persistent workgroups per batch item, the item `b` on gridDim.y.  A workgroup takes runs of BLOCK consecutive samples,
// SA_BLOCKS runs apart; every term is converted to double ONCE and multiplied into the NS sums held in double in registers.  One
// fixed-order workgroup reduction at the end (lanes by halving shuffles, then the waves in turn); every workgroup writes its NS
// doubles, also when it met no sample: sums[b][i][workgroup].
template <typename R, int D, bool HESS, typename Terms>
__device__ __forceinline__ void partial_sums(const KParams &p, const Terms &terms, double *__restrict__ sums, int64_t b)
{
    constexpr int P = params(D), M = moments(D), NS = num_sums(D, HESS), K = D * (D + 1) / 2;
    __shared__ double part[WAVES][NS];
    double acc[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) acc[i] = 0.0;
    for (int64_t o = (int64_t)blockIdx.x * BLOCK + threadIdx.x; o < p.N; o += (int64_t)SA_BLOCKS * BLOCK) {
        double od[D + 1];
        R lt, q[D], h[K];
        terms(o, od, lt, q, h);
        // one conversion to double each
        acc[0] += (double)lt;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const double qd = (double)q[d];
#pragma unroll
            for (int e = 0; e <= D; ++e) acc[1 + d * (D + 1) + e] = __builtin_fma(qd, od[e], acc[1 + d * (D + 1) + e]);
        }
        if (HESS) {
            double mo[M];
#pragma unroll
            for (int e = 0; e <= D; ++e) {
#pragma unroll
                for (int f = e; f <= D; ++f) mo[pair_index(e, f, D + 1)] = f == D ? od[e] : od[e] * od[f];
            }
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const double hk = (double)h[k];
#pragma unroll
                for (int m = 0; m < M; ++m) acc[1 + P + k * M + m] = __builtin_fma(hk, mo[m], acc[1 + P + k * M + m]);
            }
        }
    }
    // the workgroup's sums in a fixed order: lanes by halving shuffles, then the waves one after the other
#pragma unroll
    for (int i = 0; i < NS; ++i) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc[i] += __shfl_down(acc[i], off, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NS; ++i) part[wave][i] = acc[i];
    }
    __syncthreads();
    if (threadIdx.x < NS) {
        double t = part[0][threadIdx.x];
        for (int w = 1; w < WAVES; ++w) t += part[w][threadIdx.x];
        sums[(b * NS + threadIdx.x) * SA_BLOCKS + blockIdx.x] = t;
    }
}

// The other organisation of the same sums, for the instantiations whose NS accumulators leave one wave per SIMD (3-D with a
// Hessian: 256 VGPRs + 42..58 AGPRs): the 1 + D + K terms and the D + 1 indices of a run of BLOCK samples go through LDS as doubles
// (a record of REC doubles per sample), and thread (i, j) = (sum, j-th part of the run) adds its sum over its samples -- one
// accumulator per thread instead of NS, 82..176 VGPRs, 2..5 waves per SIMD, 30 KiB of LDS.  GROUPS = BLOCK / NS parts (3 in 3-D:
// 219 of the 256 threads add).  The parts are added in turn at the end.
template <typename R, int D, typename Terms>
__device__ __forceinline__ void partial_sums_staged(const KParams &p, const Terms &terms, double *__restrict__ sums, int64_t b)
{
    constexpr int P = params(D), M = moments(D), NS = num_sums(D, true), K = D * (D + 1) / 2;
    constexpr int NV = 1 + D + K, REC = NV + D + 1, GROUPS = BLOCK / NS, PER = (BLOCK + GROUPS - 1) / GROUPS;
    static_assert(GROUPS >= 1, "one thread per sum at least");
    __shared__ double stage[BLOCK * REC];
    __shared__ double part[GROUPS][NS];
    // which term and which two indices this thread multiplies
    const int grp = threadIdx.x / NS, own = threadIdx.x - grp * NS;
    int vi = 0, ea = D, eb = D;
    if (own >= 1 && own < 1 + P) { vi = 1 + (own - 1) / (D + 1); ea = (own - 1) % (D + 1); }
    if (own >= 1 + P) {
        const int k = (own - 1 - P) / M, m = (own - 1 - P) - k * M;
        vi = 1 + D + k;
        for (int e = 0; e <= D; ++e)
            for (int f = e; f <= D; ++f)
                if (pair_index(e, f, D + 1) == m) { ea = e; eb = f; }
    }
    const int s0 = grp * PER, s1 = grp < GROUPS ? (s0 + PER < BLOCK ? s0 + PER : BLOCK) : s0;
    double acc = 0.0;
    for (int64_t base = (int64_t)blockIdx.x * BLOCK; base < p.N; base += (int64_t)SA_BLOCKS * BLOCK) {
        const int64_t o = base + threadIdx.x;
        double *rec = stage + threadIdx.x * REC;
        if (o < p.N) {
            double od[D + 1];
            R lt, q[D], h[K];
            terms(o, od, lt, q, h);
            rec[0] = (double)lt;
#pragma unroll
            for (int d = 0; d < D; ++d) rec[1 + d] = (double)q[d];
#pragma unroll
            for (int k = 0; k < K; ++k) rec[1 + D + k] = (double)h[k];
#pragma unroll
            for (int e = 0; e <= D; ++e) rec[NV + e] = od[e];
        } else {
#pragma unroll
            for (int v = 0; v < REC; ++v) rec[v] = 0.0;
        }
        __syncthreads();
#pragma unroll 4
        for (int s = s0; s < s1; ++s) {
            const double *r = stage + s * REC;
            acc = __builtin_fma(r[vi], r[NV + ea] * r[NV + eb], acc);
        }
        __syncthreads();
    }
    if (grp < GROUPS) part[grp][own] = acc;
    __syncthreads();
    if (threadIdx.x < NS) {
        double t = part[0][threadIdx.x];
        for (int g = 1; g < GROUPS; ++g) t += part[g][threadIdx.x];
        sums[(b * NS + threadIdx.x) * SA_BLOCKS + blockIdx.x] = t;
    }
}

// The finish of item `b` by one workgroup: wave w sums the SA_BLOCKS doubles of the sums i = w, w + 4, ..: 16 independent partial
// sums per lane, folded in a fixed order, then the lanes by halving shuffles.  tot[NS] (shared) holds the sums after the barrier.
template <int D, bool HESS>
__device__ __forceinline__ void finish_sums(const double *__restrict__ sums, int64_t b, double *tot)
{
    constexpr int NS = num_sums(D, HESS);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = wave; i < NS; i += WAVES) {
        // FINISH_WAYS independent loads per lane, folded pairwise: which double goes into which sum is fixed
        const double *col = sums + (b * NS + i) * SA_BLOCKS;
        double a[FINISH_WAYS];
#pragma unroll
        for (int j = 0; j < FINISH_WAYS; ++j) a[j] = col[lane + 64 * j];
#pragma unroll
        for (int w = FINISH_WAYS / 2; w > 0; w /= 2) {
#pragma unroll
            for (int j = 0; j < w; ++j) a[j] += a[j + w];
        }
        double t = a[0];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
        if (lane == 0) tot[i] = t;
    }
    __syncthreads();
}

// tot -> gradient (B, D, D+1), hessian (B, P, P): BOTH triangles of the Hessian from the same sum (exactly symmetric), in R
template <typename R, int D, bool HESS>
__device__ __forceinline__ void write_gradient_hessian(const double *tot, int64_t b, R *__restrict__ gradient, R *__restrict__ hessian)
{
    constexpr int P = params(D), M = moments(D);
    if (threadIdx.x < P) gradient[b * P + threadIdx.x] = (R)tot[1 + threadIdx.x];
    if (HESS) {
        for (int t = threadIdx.x; t < P * P; t += BLOCK) {
            const int row = t / P, col = t - row * P;
            const int d = row / (D + 1), e = row - d * (D + 1), d2 = col / (D + 1), e2 = col - d2 * (D + 1);
            const int k = pair_index(d < d2 ? d : d2, d < d2 ? d2 : d, D);
            const int m = pair_index(e < e2 ? e : e2, e < e2 ? e2 : e, D + 1);
            hessian[b * P * P + t] = (R)tot[1 + P + k * M + m];
        }
    }
}

// the bytes of the sums of the call WITH a Hessian: a function of the problem alone
static int64_t sa_workspace(int D, int B) { return (int64_t)B * num_sums(D, true) * SA_BLOCKS * (int64_t)sizeof(double); }

} // namespace ssd_affine
} // namespace ip
