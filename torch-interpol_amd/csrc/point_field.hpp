// ===========================================================================
// point_field.hpp -- what the kernels with one thread per sample of a point-by-point field (B, *shape, K) share: the
// K-component element and the map from a thread to its sample.  Included by compose.hip, ssd.hip, lcc.hip and mi.hip.
// ===========================================================================
#pragma once
#include "ops_generic.hpp"
#include <stdint.h>

namespace ip {

// D components of one lattice point; alignment of a single component
template <typename R, int D> struct PointVec { R c[D]; };
static_assert(alignof(PointVec<float, 3>) == 4 && sizeof(PointVec<float, 3>) == 12, "point-by-point element: 4-byte aligned");
static_assert(alignof(PointVec<double, 3>) == 8 && sizeof(PointVec<double, 3>) == 24, "point-by-point element: 8-byte aligned");

// Which sample a thread of the forward kernel owns.  D < 3: the samples in storage order, 256 per workgroup.  D == 3: a workgroup
// owns a 4 x 2 x 32 box of samples (z fastest: a wave is two rows of 32), so that the stencils of a wave under a rough field
// overlap in two dims instead of lying along one row.  Measured on 1 x 256^3 x 3 float32, order 1: i.i.d. sigma = 2 field
// 0.70 -> 0.49 ms, smooth field 0.21 -> 0.24 ms (the row pieces of `right` / `out` are 384 B instead of 768 B); boxes of
// 4 x 4 x 16, 2 x 4 x 32 and 2 x 8 x 16 were within 5 % on the rough field and no better on the smooth one, 4 x 8 x 8 slower
// on both (profiles/compose.txt).
constexpr int BOX_Z = 32, BOX_Y = 2, BOX_X = BLOCK / (BOX_Z * BOX_Y);

// ... as the thread of workgroup `bi` out of compose_blocks (a kernel whose workgroups loop over the boxes: mi.hip)
template <int D>
__device__ __forceinline__ int64_t compose_sample(const KParams &p, unsigned bi)
{
    if (D == 3) {
        const unsigned nz = ((unsigned)p.gshape[2] + BOX_Z - 1) / BOX_Z, ny = ((unsigned)p.gshape[1] + BOX_Y - 1) / BOX_Y;
        const unsigned bz = bi % nz; bi /= nz;
        const unsigned by = bi % ny, bx = bi / ny;
        const unsigned z = bz * BOX_Z + threadIdx.x % BOX_Z, y = by * BOX_Y + (threadIdx.x / BOX_Z) % BOX_Y,
                       x = bx * BOX_X + threadIdx.x / (BOX_Z * BOX_Y);
        if (z >= (unsigned)p.gshape[2] || y >= (unsigned)p.gshape[1] || x >= (unsigned)p.gshape[0]) return -1;
        return ((int64_t)x * p.gshape[1] + y) * p.gshape[2] + z;
    }
    const int64_t o = (int64_t)bi * BLOCK + threadIdx.x;
    return o < p.N ? o : -1;
}
template <int D>
__device__ __forceinline__ int64_t compose_sample(const KParams &p) { return compose_sample<D>(p, blockIdx.x); }

// workgroups of compose_fwd along x
template <int D>
static int64_t compose_blocks(const KParams &k)
{
    if (D == 3)
        return (((int64_t)k.gshape[0] + BOX_X - 1) / BOX_X) * (((int64_t)k.gshape[1] + BOX_Y - 1) / BOX_Y) * (((int64_t)k.gshape[2] + BOX_Z - 1) / BOX_Z);
    return (k.N + BLOCK - 1) / BLOCK;
}

} // namespace ip
