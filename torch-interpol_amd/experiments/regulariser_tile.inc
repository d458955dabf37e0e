// ===========================================================================
// regulariser_tile.inc -- (experiment, measured slower: experiments/README.md, profiles/regulariser.txt) L v of the
// regulariser from an LDS halo tile.  Included at the end of csrc/regulariser.hip under IP_EXPERIMENTS (`make experiments`).
//
// 3-D, float32, every bound but dst1.  A workgroup of 256 threads owns a box of 8 x 8 x 32 lattice points (z contiguous).  It
// stages the box plus its 2-ring halo once -- 12 x 12 x 36 points, the three components in planes of their own, 62 208 bytes:
// two workgroups per CU -- with the bound resolved while staging: the staged value is sign_x sign_y sign_z f[wrap(x, y, z)], so
// the 25 taps are read with compile-time offsets and wave-uniform coefficients.  (dst1 is left out: its sign 0 at index 0
// applies to the axis of a stencil only, an in-range point has no single staged value.)  Thread (y, z) computes the 8 outputs
// of its x-column; consecutive lanes read consecutive z: no bank conflicts.
// ===========================================================================
namespace ip {
namespace reg {

constexpr int TB0 = 8, TB1 = 8, TB2 = 32;                            // outputs per tile
constexpr int TH0 = TB0 + 4, TH1 = TB1 + 4, TH2 = TB2 + 4;           // with the halo
static_assert(TB1 * TB2 == BLOCK, "one thread per (y, z) of the tile");

template <int MODE>
__global__ __launch_bounds__(BLOCK) void reg_tile(KParams p, Weights<float> w, const float *__restrict__ field, float *__restrict__ out,
                                                  int B, int t1, int t2)
{
    typedef PointVec<float, 3> V;
    constexpr bool ABS = (MODE & M_ABS) != 0, MEM = (MODE & M_MEM) != 0, BEND = (MODE & M_BEND) != 0;
    __shared__ float tile[3][TH0][TH1][TH2];
    const int tz = blockIdx.x % t2, ty = (blockIdx.x / t2) % t1, tx = blockIdx.x / (t2 * t1);
    const int x0 = tx * TB0, y0 = ty * TB1, z0 = tz * TB2;
    const int z = threadIdx.x % TB2, y = threadIdx.x / TB2;
    // wave-uniform coefficients (the tables of reg_at without signs)
    const float cen = (ABS ? w.abs : 0.f) + w.axis[0][0] + w.axis[1][0] + w.axis[2][0]
                      + (BEND ? w.bend2 * (w.a1[0][0] * w.a1[1][0] + w.a1[0][0] * w.a1[2][0] + w.a1[1][0] * w.a1[2][0]) : 0.f);
    float c1[3], c2[3], cd[3][3];
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        float side = 0.f;
#pragma unroll
        for (int f = 0; f < 3; ++f) if (f != e) side += w.a1[f][0];
        c1[e] = w.axis[e][1] + (BEND ? w.bend2 * side * w.a1[e][1] : 0.f);
        c2[e] = w.axis[e][2];
#pragma unroll
        for (int f = 0; f < 3; ++f) cd[e][f] = w.bend2 * (w.a1[e][1] * w.a1[f][1]);
    }
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        const V *ub = reinterpret_cast<const V *>(field + b * p.vol_sb);
        __syncthreads();                                             // (the previous item's reads are done)
        for (int h = threadIdx.x; h < TH0 * TH1 * TH2; h += BLOCK) {
            const int hz = h % TH2, hy = (h / TH2) % TH1, hx = h / (TH2 * TH1);
            const int g[3] = { x0 + hx - 2, y0 + hy - 2, z0 + hz - 2 };
            unsigned off = 0;
            float s = 1.f;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                int idx = g[d];
                if ((unsigned)idx >= (unsigned)p.vol_n[d]) {
                    const long long pk = wrap_outofline(p.bound[d], idx, p.vol_n[d]);
                    idx = (int)(pk & 0xffffffffll);
                    s *= (float)(int)(pk >> 32);
                }
                off += (unsigned)idx * (unsigned)p.vol_ss[d];
            }
            const V v = ld_tap(ub, off);
            tile[0][hx][hy][hz] = s * v.c[0];
            tile[1][hx][hy][hz] = s * v.c[1];
            tile[2][hx][hy][hz] = s * v.c[2];
        }
        __syncthreads();
        if (y0 + y >= p.vol_n[1] || z0 + z >= p.vol_n[2]) continue;
#pragma unroll
        for (int x = 0; x < TB0; ++x) {
            if (x0 + x >= p.vol_n[0]) break;
            V r;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
#define TL(dx, dy, dz) tile[c][x + 2 + (dx)][y + 2 + (dy)][z + 2 + (dz)]
                float acc = cen * TL(0, 0, 0);
                if (MEM || BEND) {
                    acc = fma_(c1[0], TL(-1, 0, 0) + TL(1, 0, 0), acc);
                    acc = fma_(c1[1], TL(0, -1, 0) + TL(0, 1, 0), acc);
                    acc = fma_(c1[2], TL(0, 0, -1) + TL(0, 0, 1), acc);
                }
                if (BEND) {
                    acc = fma_(c2[0], TL(-2, 0, 0) + TL(2, 0, 0), acc);
                    acc = fma_(c2[1], TL(0, -2, 0) + TL(0, 2, 0), acc);
                    acc = fma_(c2[2], TL(0, 0, -2) + TL(0, 0, 2), acc);
                    acc = fma_(cd[0][1], (TL(-1, -1, 0) + TL(1, 1, 0)) + (TL(-1, 1, 0) + TL(1, -1, 0)), acc);
                    acc = fma_(cd[0][2], (TL(-1, 0, -1) + TL(1, 0, 1)) + (TL(-1, 0, 1) + TL(1, 0, -1)), acc);
                    acc = fma_(cd[1][2], (TL(0, -1, -1) + TL(0, 1, 1)) + (TL(0, -1, 1) + TL(0, 1, -1)), acc);
                }
#undef TL
                r.c[c] = w.h2[c] * acc;
            }
            const int64_t o = ((int64_t)(x0 + x) * p.vol_n[1] + (y0 + y)) * p.vol_n[2] + (z0 + z);
            *reinterpret_cast<V *>(out + b * p.val_sb + o * 3) = r;
        }
    }
}

static int reg_tile_entry(const interpol_problem *p, const void *field, void *out, double absolute, double membrane, double bending,
                          const double *voxel_size, void *stream)
{
    KParams k; int B;
    const int rc = reg_params(p, true, &k, &B);
    if (rc) return rc;
    if (k.dim != 3) return INTERPOL_E_DIM;
    if (p->dtype != INTERPOL_F32) return INTERPOL_E_DTYPE;
    for (int d = 0; d < 3; ++d) if (k.bound[d] == B_DST1) return INTERPOL_E_BOUND;
    WeightsEL<double> wd;
    const int mode = reg_weights(3, absolute, membrane, bending, 0.0, 0.0, 0, voxel_size, &wd);
    if (mode < 0) return mode;
    if (!field || !out) return INTERPOL_E_NULL;
    const uint64_t item = (uint64_t)k.N * 3 * 4;
    if (ranges_overlap(field, (uint64_t)(B - 1) * (uint64_t)k.vol_sb * 4 + item, out, (uint64_t)(B - 1) * (uint64_t)k.val_sb * 4 + item))
        return INTERPOL_E_STRIDE;
    const int t0 = (k.vol_n[0] + TB0 - 1) / TB0, t1 = (k.vol_n[1] + TB1 - 1) / TB1, t2 = (k.vol_n[2] + TB2 - 1) / TB2;
    if ((int64_t)t0 * t1 * t2 > 0x7fffffff) return INTERPOL_E_SHAPE;
    const Weights<float> w = narrow<float>(wd);
    const dim3 grid((unsigned)(t0 * t1 * t2), (unsigned)(B < 65535 ? B : 65535), 1);
    hipStream_t st = (hipStream_t)stream;
#define IP_TILE(M) case M: hipLaunchKernelGGL((reg_tile<M>), grid, dim3(BLOCK), 0, st, k, w, (const float *)field, (float *)out, B, t1, t2); break
    switch (mode) { IP_TILE(1); IP_TILE(2); IP_TILE(3); IP_TILE(4); IP_TILE(5); IP_TILE(6); default: IP_TILE(7); }
#undef IP_TILE
    return hipGetLastError() == hipSuccess ? 0 : INTERPOL_E_LAUNCH;
}

} // namespace reg
} // namespace ip

extern "C" int interpol_regulariser_tile(const interpol_problem *p, const void *field, void *out, double absolute, double membrane,
                                         double bending, const double *voxel_size, void *stream)
{
    return ip::reg::reg_tile_entry(p, field, out, absolute, membrane, bending, voxel_size, stream);
}
