// ===========================================================================
// owner_geom.hpp -- the brick geometry of the owner-computes push (push_owner.hip): bricks of first-tap cells per dim, their
// boxes, the colours, and which slots of a box its brick is the FIRST colour launch to write.  Plain C++: device code, host code
// and the GPU-less check of the geometry (tests/native/first_writer_geom.cpp) read the same functions.
// ===========================================================================
#pragma once

#ifdef __HIPCC__
#define IP_GEOM_HD __host__ __device__ __forceinline__
#else
#define IP_GEOM_HD inline
#endif

namespace ip {
namespace owner {

constexpr int BR = 16;                          // brick edge, in first-tap cells
constexpr int OFF = 160;                        // first taps in [-OFF, n + OFF) are binned (a zoom by 2 about the centre of a 256^3 lattice reaches 128 voxels
                                                // beyond it); beyond: scattered directly
constexpr int BOX = BR + 3;                     // lattice points a brick's stencils touch per dim (K <= 3)

// Bricks of first-tap cells, per dim.  INTERIOR cells [lo, top) lie in nin bricks of BR cells: the bricks up to index
// `split` are aligned to lo, the ones above it to top (brick `split` is the short one in between).  Two cases:
//   * the boundary condition of the dim is a single reflection or a clamp without a change of sign (replicate, dct1, dct2) and
//     the lattice is not tiny: lo = -9, top = n + 6 -- the boxes of the bricks at the two ends leave the lattice by at most 9
//     points: their contents are FOLDED back inside the box in LDS before the flush, and that far out the target of every fold
//     still lies in the same box (low end: box [-9, 10), point -9 -> 8; high end: box [n - 10, n + 9), point n + 8 -> n - 9);
//   * else: lo = 0, top = n - K -- the stencils that lie inside the lattice (split = nin - 1: the last brick holds the remainder).
// [lo - OFF, lo) lies in NLO bricks, [top, top + NHI * BR) in NHI bricks: the SHELL (stencils far outside the lattice, wrapping and
// sign-changing boundary conditions), whose bricks flush through the boundary tables with global atomics -- their boxes alias.
constexpr int NLO = OFF / BR, NHI = (OFF + 3 + BR - 1) / BR;
struct BrickGrid {
    int nb[3];                                  // bricks per dim
    int lo[3], top[3], nin[3], split[3];        // interior first-tap cells [lo, top), bricks that hold them, the short brick
    int per_item;                               // nb[0] * nb[1] * nb[2]
    int item;                                   // brick-index stride of a batch item: per_item, or 0 when the items share ONE target (their bricks are the same)
    int capd;                                   // descriptors (runs) per brick: CAPD, CAPX for a shared target (every item's tiles feed the brick)
};
// dim d of the grid: spline order K, n lattice points, f: the dim folds (push_owner.hip: folds)
IP_GEOM_HD void brick_grid_dim(BrickGrid &g, int d, int K, int n, bool f)
{
    // folding dims: as far out as the mirror image of every point of the end bricks' boxes stays inside the box
    g.lo[d] = f ? -(BOX - 1) / 2 : 0;
    g.top[d] = f ? n - (BOX + 1) / 2 + BR : (n - K > 0 ? n - K : 0);
    g.nin[d] = (g.top[d] - g.lo[d] + BR - 1) / BR;
    if (f) {
        // no short brick of less than K cells: the box of the brick below it (K points beyond its own cells) must not
        // reach the brick above it, which has the same colour
        const int c = g.top[d] - g.lo[d] - BR * (g.nin[d] - 1);
        if (c < K) { g.top[d] -= c; g.nin[d] -= 1; }
    }
    g.split[d] = f ? g.nin[d] / 2 : (g.nin[d] > 0 ? g.nin[d] - 1 : 0);
    g.nb[d] = NLO + g.nin[d] + NHI;
}
// brick of a first-tap cell (inside [lo - OFF, top + NHI * BR)) and the cell's index inside its brick (<< 16)
IP_GEOM_HD int brick_and_cell(int ft, int lo, int top, int nin, int split)
{
    if (ft < lo) return ((ft - lo + OFF) >> 4) | (((ft - lo + OFF) & (BR - 1)) << 16);
    if (ft >= top) return (NLO + nin + ((ft - top) >> 4)) | (((ft - top) & (BR - 1)) << 16);
    const int u = ft - lo, v = top - 1 - ft;
    const bool hi = u >= BR * split && (v >> 4) < nin - 1 - split;
    return hi ? (NLO + nin - 1 - (v >> 4)) | ((BR - 1 - (v & (BR - 1))) << 16) : (NLO + (u >> 4)) | ((u & (BR - 1)) << 16);
}
// first cell of a brick
IP_GEOM_HD int brick_origin(int bk, int lo, int top, int nin, int split)
{
    if (bk < NLO) return lo + bk * BR - OFF;
    if (bk >= NLO + nin) return top + (bk - NLO - nin) * BR;
    const int j = bk - NLO;
    return j <= split ? lo + j * BR : top - (nin - j) * BR;
}

// first brick index a launch enumerates along dim d: a colour 0 .. 7 takes the interior bricks whose index has the parity of its bit
// 2 - d, two apart (their boxes are disjoint); the other launches enumerate every brick
IP_GEOM_HD int color_first(int color, int d)
{
    if (color >= 8) return 0;
    const int par = (color >> (2 - d)) & 1;
    return NLO + ((par - NLO) & 1);                                  // first interior brick index of that parity
}
// ... and the bit of a dim in the colour that launches interior brick bk of it: color_first has the parity of the bit, the step is 2
IP_GEOM_HD int color_bit(int bk) { return bk & 1; }

// FIRST WRITER.  The colours run in the order 0 .. 7 and the box of a brick overlaps, across dim d, the boxes of its two neighbours
// in d alone (bricks two apart: disjoint).  A slot that lies in the overlap of the dims D has the earlier writers c ^ mask(S), S in D,
// so it has none exactly when no dim of D has its bit set in c: an interior brick bk is the first colour launch to write the slots
// [f_lo, f_hi) of dim d -- FRESH with respect to d -- and a slot of the box is fresh when it is in all three dims.  Bit clear: the
// whole dim (both neighbours in d come later).  Bit set: what neither neighbour's box covers, from the origins -- a short brick at
// `split` overlaps by more than the 3 slots of a regular one, and the range may be empty.  A side without an interior neighbour
// borders a shell brick, which flushes in the shell launch, after every colour: fresh.  (dst1 takes the first interior brick out of
// the colours as well: the overlap with it counts all the same -- fewer fresh slots than there are is always correct.)
IP_GEOM_HD void fresh_range(int bk, int d, const BrickGrid &g, int &f_lo, int &f_hi)
{
    f_lo = 0; f_hi = BOX;
    const int j = bk - NLO;
    if (j < 0 || j >= g.nin[d] || !color_bit(bk)) return;
    const int o = brick_origin(bk, g.lo[d], g.top[d], g.nin[d], g.split[d]);
    if (j > 0) f_lo = brick_origin(bk - 1, g.lo[d], g.top[d], g.nin[d], g.split[d]) + BOX - o;
    if (j + 1 < g.nin[d]) f_hi = brick_origin(bk + 1, g.lo[d], g.top[d], g.nin[d], g.split[d]) - o;
    f_lo = f_lo < 0 ? 0 : (f_lo > BOX ? BOX : f_lo);
    f_hi = f_hi < 0 ? 0 : (f_hi > BOX ? BOX : f_hi);
}

// the interior bricks [k_lo, k_hi] of dim d whose box holds lattice point x (k_lo > k_hi: none)
IP_GEOM_HD void bricks_over(int x, int d, const BrickGrid &g, int &k_lo, int &k_hi)
{
    k_lo = 0; k_hi = -1;
    if (g.nin[d] <= 0 || x < g.lo[d]) return;
    const int cell = x < g.top[d] ? x : g.top[d] - 1;
    k_hi = brick_and_cell(cell, g.lo[d], g.top[d], g.nin[d], g.split[d]) & 0xffff;
    if (brick_origin(k_hi, g.lo[d], g.top[d], g.nin[d], g.split[d]) + BOX <= x) { k_hi = -1; return; }
    k_lo = k_hi;
    while (k_lo > NLO && brick_origin(k_lo - 1, g.lo[d], g.top[d], g.nin[d], g.split[d]) + BOX > x) --k_lo;
}

} // namespace owner
} // namespace ip
