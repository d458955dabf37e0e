/* ===========================================================================
 * interpol_hip.h -- C-ABI of libinterpol_hip.so, the MI355X (gfx950) kernels
 * behind the torch-interpol hot path.
 *
 * The reference (balbasty/torch-interpol @2024_10_08) has no FFI: its operator
 * seam is the Python module interpol/pushpull.py.  Each entry point below is
 * what a binding for that seam would call; the reference interface it
 * replaces is cited on every declaration.  INTEGRATION.md shows the ctypes
 * stub a maintainer of the reference would add.
 *
 * Conventions
 *   - plain C types only: device pointers, sizes, element strides, int codes;
 *   - the caller owns every buffer (inputs, outputs, scratch); the library
 *     never retains a pointer to them.  State: the ONLY state of the library
 *     lives in csrc/defer.hip.  The tile hand-back (see interpol_set_handback
 *     below): 1 KiB of pinned host memory per device on first use, and up to 16
 *     slots of 3 MiB of device memory per device, one per stream whose launches
 *     met stretched tiles -- recycled least-recently-used, released by
 *     interpol_release_stream(), freed at process exit.  The item chains of the
 *     owner-computes push (INTERPOL_FLAG_SERIAL_ITEMS below): one non-blocking
 *     side stream and two events per device, created by the first call that
 *     forks, shared by all callers (a mutex covers the enqueueing of one call),
 *     destroyed at process exit;
 *   - kernels are enqueued asynchronously on `stream` (a hipStream_t passed as
 *     void*; NULL = the default stream); no internal synchronisation (what a
 *     call enqueues on the side stream is joined into `stream` before it returns);
 *   - return value: 0 = ok, < 0 = INTERPOL_E_* (invalid argument, nothing
 *     launched), > 0 = a hipError_t raised by the launch (the *_affine,
 *     interpol_compose* and interpol_jac* entry points return negative codes only: INTERPOL_E_LAUNCH);
 *   - boundary codes 0..6 = zero, replicate, dct1, dct2, dst1, dst2, dft
 *     (reference interpol/bounds.py:8-15); spline orders 0..7
 *     (interpol/splines.py:7-15); extrapolate 0 = no, 1 = yes, 2 = hist
 *     (interpol/bounds.py:18-21).
 * =========================================================================== */
#ifndef INTERPOL_HIP_H
#define INTERPOL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define INTERPOL_ABI_VERSION 1

/* storage types of image tensors / coordinate tensors */
enum {
    INTERPOL_F32  = 0,   /* float  storage, float math                        */
    INTERPOL_F64  = 1,   /* double storage, double math (coords must be F64)  */
    INTERPOL_BF16 = 2,   /* bf16 storage, float math   (coords must be F32)   */
    INTERPOL_F16  = 3    /* half storage, float math   (coords must be F32)   */
};

/* error codes (negative) */
enum {
    INTERPOL_OK          =  0,
    INTERPOL_E_DIM       = -1,   /* dim not in 1..3                            */
    INTERPOL_E_ORDER     = -2,   /* spline order not in 0..7 (splines.py:80)   */
    INTERPOL_E_BOUND     = -3,   /* bound code not in 0..6                     */
    INTERPOL_E_DTYPE     = -4,   /* unsupported dtype combination              */
    INTERPOL_E_SHAPE     = -5,   /* non-positive / too large extent            */
    INTERPOL_E_NULL      = -6,   /* required pointer is NULL                   */
    INTERPOL_E_EXTRAP    = -7,   /* extrapolate not in 0..2                    */
    INTERPOL_E_PREFILTER = -8,   /* prefilter bound dst1/dst2 (coeff.py:243)   */
    INTERPOL_E_SCRATCH   = -9,   /* scratch buffer too small                   */
    INTERPOL_E_STRIDE    = -10,  /* stride pattern not supported (see below)   */
    INTERPOL_E_LAUNCH    = -11   /* a kernel launch failed (the *_affine, interpol_compose* and interpol_jac* entry points, which return no hipError_t) */
};

/* ---------------------------------------------------------------------------
 * Problem descriptor shared by all sampling operators.
 *
 *   "vol"  = the lattice that is INDEXED by the coordinates: the input image of
 *            pull/grad/hess, the target image of push/count/pushgrad.
 *            Layout (batch, channel, *vol_shape); any element strides.
 *   "grid" = the coordinates, layout (batch, *grid_shape, dim); component d
 *            addresses vol spatial dim d, in voxels (nd.py:44).
 *   "val"  = the per-sample values: the output of pull/grad/hess, the input of
 *            push/pushgrad.  Layout (batch, channel, *grid_shape[, dim[, dim]]).
 *
 * A batch stride of 0 broadcasts that tensor over the batch (api.py:122-126).
 * Strides are in ELEMENTS.  Unused trailing entries (dim < 3) are ignored.
 * Supported patterns (else INTERPOL_E_STRIDE): gather sources (vol of pull/grad/
 * hess) may have ANY non-negative strides; grid and val must be row-major
 * contiguous over their spatial (+component) dims with free batch/channel
 * strides; scatter targets (vol of push/count/pushgrad) must be dense, except
 * that a batch stride of 0 makes ONE shared (C, *shape) target into which every
 * batch item is accumulated (= grid_push(...).sum(0) of the reference).
 * One (batch, channel) image of vol must span < 4 GiB (32-bit byte offsets).
 * --------------------------------------------------------------------------- */
typedef struct interpol_problem {
    int32_t abi_version;        /* INTERPOL_ABI_VERSION                        */
    int32_t dim;                /* D in 1..3                                   */
    int32_t dtype;              /* INTERPOL_* of vol and val                   */
    int32_t grid_dtype;         /* INTERPOL_F32 or INTERPOL_F64                */
    int32_t extrapolate;        /* 0, 1, 2                                     */
    int32_t bound[3];           /* per spatial dim                             */
    int32_t order[3];           /* per spatial dim                             */
    int32_t flags;              /* INTERPOL_FLAG_*                             */
    int64_t batch;              /* B = max over tensors                        */
    int64_t channels;           /* C                                           */
    int64_t vol_shape[3];
    int64_t grid_shape[3];
    int64_t vol_stride[5];      /* batch, channel, s0, s1, s2                  */
    int64_t grid_stride[5];     /* batch, s0, s1, s2, component                */
    int64_t val_stride[7];      /* batch, channel, s0, s1, s2, d, e            */
} interpol_problem;

/* flags */
#define INTERPOL_FLAG_NO_FASTPATH   1   /* force the generic kernels (testing)           */
#define INTERPOL_FLAG_ACCUMULATE    2   /* push/count/pushgrad: do not zero the target (fp32 / fp64 targets only:
                                           INTERPOL_E_DTYPE for bf16 / f16, which are narrowed once) */
#define INTERPOL_FLAG_FORCE_TILED   4   /* take the LDS-tiled kernel wherever one exists (testing) */
/* Separable (tensor-product) coordinates, the grids of resize / restrict (resize.py:96-123,
 * restrict.py:88-117: `stack(meshgrid_ij(*lin), -1)`): `grid` points to the D coordinate vectors
 * lin_0 (grid_shape[0] values), lin_1, lin_2 stored back to back (grid_dtype); sample
 * (o_0, o_1, o_2) has coordinates (lin_0[o_0], lin_1[o_1], lin_2[o_2]) for every batch item.
 * grid_stride is ignored; no (B,*out,D) grid is read (-12 B/sample in 3-D).  The backward
 * entry points accept it only when grad_grid is not requested (else INTERPOL_E_STRIDE). */
#define INTERPOL_FLAG_SEPARABLE_GRID 8
/* `grid` holds DISPLACEMENTS in voxels, layout as a dense grid: the coordinates are
 * o_d + grid[b, o, d], the identity lattice being added in registers -- the fused form of
 * add_identity_grid_ (api.py:490-513) followed by the operator; same rounding (one float add of
 * the exactly representable index).  grad_grid of the backward entry points is then the
 * gradient w.r.t. the displacement (identical values).  Not combinable with SEPARABLE_GRID. */
#define INTERPOL_FLAG_DISPLACEMENT  16
/* interpol_push only: the target has channels + 1 channels, (B, C+1, *shape); channel C receives
 * the COUNT image (what interpol_count writes: the splatted ones, pushpull.py:106-142) in the same
 * pass over the grid -- push followed by count on the same grid is the usual pairing (normalised
 * splatting; SURVEY config 4).  vol_stride describe the (B, C+1, *shape) target. */
#define INTERPOL_FLAG_WITH_COUNT    32
/* interpol_push / interpol_count: organise the scatter OWNER-COMPUTES (push_owner.hip): the samples are
 * first sorted by the 16^3 brick of target lattice points their first tap falls into (one pass over the
 * inputs), then every brick is accumulated in LDS by one workgroup and added to the target with plain
 * loads and stores -- no global atomics: under replicate / dct1 / dct2 the stencils that leave the lattice
 * are folded back inside the LDS box of the brick at the end of the dim; what lies further out than 9
 * points, and the other boundary conditions, flush a thin shell of bricks with atomics.  The cost hardly
 * depends on the deformation (4x2x256^3 cubic: 2.8 - 3.6 ms from the identity to i.i.d. noise of sigma = 6
 * voxels), where the sample-stationary tiles need the stencils of a 16^3 tile of samples to fit a
 * 33 x 33 x 32 LDS box (2.2 ms at the identity, 3.5 at sigma = 2, 126 at sigma = 6).
 * 3-D, one order 1..3 or -- round 6 -- any mix of orders 1..3 on a dense grid (the cubic's bricks with every dim's own first tap and
 * weights: [1,2,3] at sigma = 6, 4x2x256^3: 3.9 ms where the tiles took 72; the gathers of interpol_pull_ws / interpol_grad_ws / the
 * backward passes likewise) (trilinear since round 5: 4x2x256^3, 2.3 - 3.1 ms from the identity to sigma = 6, where its tiles take
 * 1.3 - 16 ms; all orders 0, nearest neighbour, through the same bricks with the box held in FLOATS -- round 6: no fixed point at order
 * 0, one LDS float add per sample and channel, so a lattice point hit by one sample holds that sample's value bit for bit and a
 * non-finite source stays on its own lattice point, like iso0.py:65-118 -- 2.5 - 2.9 ms; under AUTO the probe chooses between the bricks
 * and the generic kernel's global atomics), float32 coordinates.  Needs the workspace announced by
 * interpol_scatter_workspace(); ignored (tiles / generic kernels) when it does not apply.
 *   INTERPOL_FLAG_BINNED_SCATTER: always;
 *   INTERPOL_FLAG_AUTO_SCATTER:   a probe kernel of the same call examines 128 tiles of the sample grid
 *     (owner-computes when samples fall outside the tiles' boxes, or -- two channels and more -- when
 *     roughness makes those boxes large) and writes a device-side gate; both organisations are enqueued, each kernel reads the gate on
 *     entry and one of the two returns at once (about 50 us of empty launches).  Stateless: the choice
 *     depends on the coordinates of this call alone; safe under hipGraph capture. */
#define INTERPOL_FLAG_BINNED_SCATTER 64
#define INTERPOL_FLAG_AUTO_SCATTER  (1 << 24)
/* (experimental, opt-in) interpol_pull_ws with the single-pass small-box tiles for smooth deformations in front of the class-sorted
 * tiles (pull_direct.hip): measured slower than the class-sorted tiles alone at config 2 (identity 1.16 against 1.05 ms, mixed
 * fields up to +26 %: profiles/r04_pull_steps.txt), so it is not the default. */
#define INTERPOL_FLAG_SMALL_TILES (1 << 25)
/* interpol_push / interpol_count through the owner-computes organisation: keep every batch item on the caller's stream.  By default a
 * call with a target per batch item and at least two items runs the items as two concurrent chains (zero-fill of the items' targets,
 * own_bin, colour launches, shell launch): the first half of the batch on the caller's stream, the second on a side stream that the library
 * keeps per device, forked behind the probe and joined before the call returns, so the caller's stream sees the same ordering as before (push_owner.hip:
 * ITEM CHAINS; "State" below).  A shared target, a single item and a stream that is being captured into a hipGraph take the single-stream
 * schedule anyway.  The results of the two schedules are the same: this flag exists so that both can be timed in one process. */
#define INTERPOL_FLAG_SERIAL_ITEMS (1 << 26)
/* interpol_push / interpol_count through the owner-computes organisation: launch the GENERAL instantiation of own_accumulate for every
 * colour.  By default the eight colour launches of orders 1 / 2 / 3 run an instantiation without the paths that only the shell launch
 * takes (atomic flush, boundary tables, candidate scan) and with the rare per-brick modes (64-bit sums of a dense brick, float atomics
 * for non-finite sources) unswitched out of its tap loop (push_owner.hip: own_accumulate, SHELL = false).  Same expressions in the same
 * order: the results are the same wherever the general kernel is reproducible.  This flag exists so that both can be timed and compared
 * in one process (tools/ab_lean.py, tests/test_lean_kernels.py); the Python API never sets it. */
#define INTERPOL_FLAG_GENERAL_KERNELS (1 << 27)
/* interpol_push / interpol_count through the owner-computes organisation: publish EVERY run of a shell brick.  By default a sample tile
 * that holds at most 16 samples in shell bricks altogether (push_owner.hip: THIN_SHELL_RUN) publishes no run for them: own_bin scatters
 * those samples itself with float atomics, a wave per sample and a stencil tap per lane, so a handful of stray samples far outside the
 * lattice -- the 4 sigma tail of a rough field at the faces of the volume -- no longer costs every call a shell launch that scans all the
 * bricks and runs a whole brick chain per stray.  A tile with more shell samples (a zoom, a rotation, a non-folding bound) publishes its
 * runs as before.  Only shell bricks are concerned, which flush with float atomics either way: the interior stays bit-reproducible and
 * both sides agree bit for bit outside the stencils of the samples concerned.  This flag exists so that both can be timed and compared
 * in one process (tools/ab_shell_runs.py, tests/test_stray_shell_samples.py); the Python API never sets it. */
#define INTERPOL_FLAG_SHELL_RUNS (1 << 28)
/* interpol_push / interpol_count through the owner-computes organisation: flush EVERY lattice point of a brick's box with load + add +
 * store.  By default a colour launch of orders 1 / 2 / 3 stores, without a load, the points of its box that no earlier colour's box
 * holds (push_owner.hip: own_accumulate, first writer; owner_geom.hpp: fresh_range) -- the load would return the zero of the call's own
 * zero-fill, and 0.f + x == x.  That needs the call to zero-fill the target (never under INTERPOL_FLAG_ACCUMULATE), a target per batch
 * item (not a shared one), and a brick that own_bin's direct scatters (stray and far samples: float atomics in front of the colours)
 * did not write under: own_bin marks those bricks, one word per brick of the workspace, and they keep load + add + store.  The results
 * are the same bit for bit wherever the push is reproducible.  This flag exists so that both can be timed and compared in one process
 * (tools/ab_first_writer.py, tests/test_first_writer_flush.py); the Python API never sets it. */
#define INTERPOL_FLAG_RMW_FLUSH (1 << 29)
/* The sample coordinates are an AFFINE function of the sample index, x = A o + t -- the fused form of
 * affine_grid (api.py:534-572) followed by the operator: `grid` points to ONE D x (D+1) matrix [A | t]
 * (grid_dtype, row-major), evaluated in registers as ((A_d0 o_0) + A_d1 o_1 ...) + t_d with fused
 * multiply-adds; grid_stride is ignored and no (B,*out,D) grid is read (-4 D bytes per sample).  Not
 * combinable with SEPARABLE_GRID / DISPLACEMENT.  There is no per-sample grad_grid (INTERPOL_E_STRIDE from
 * interpol_pull_backward / interpol_push_backward[_ws] / interpol_count_backward, like SEPARABLE_GRID), but
 * the MATRIX is differentiable through pull, push and count: interpol_pull_backward_affine /
 * interpol_push_backward_affine below reduce the per-sample grid gradient against the sample index on chip
 * and return the D x (D+1) gradient of [A | t].  What still goes through the dense lattice (affine_grid
 * followed by the operator): grid_grad with a matrix that needs a gradient, a batch of matrices (one per
 * item), and derivatives of third order and beyond. */
#define INTERPOL_FLAG_AFFINE_GRID   128

/* --- forward operators -------------------------------------------------------
 * interpol_pull      replaces pushpull.grid_pull      (interpol/pushpull.py:35-66;
 *                    nd.pull nd.py:80-143, iso1.pull*d, iso0.pull*d)
 *                    vol (B,C,*in) , grid (B,*out,D) -> val (B,C,*out)
 * interpol_push      replaces pushpull.grid_push      (pushpull.py:70-102; nd.push nd.py:146-213)
 *                    val (B,C,*in) , grid (B,*in,D)  -> vol (B,C,*shape), zero-filled here
 *                    unless INTERPOL_FLAG_ACCUMULATE
 * interpol_count     replaces pushpull.grid_count     (pushpull.py:106-142)
 *                    grid (B,*in,D) -> vol (B,1,*shape)     (p->channels must be 1)
 * interpol_grad      replaces pushpull.grid_grad      (pushpull.py:146-172; nd.grad nd.py:216-288)
 *                    vol , grid -> val (B,C,*out,D)
 * interpol_pushgrad  replaces pushpull.grid_pushgrad  (pushpull.py:176-203; nd.pushgrad nd.py:291-364)
 *                    val (B,C,*in,D) , grid -> vol (B,C,*shape)
 * interpol_hess      replaces pushpull.grid_hess      (pushpull.py:207-233; nd.hess nd.py:367-464)
 *                    vol , grid -> val (B,C,*out,D,D)
 *
 * Low-precision scatter: for dtype BF16/F16 the push-type operators need a
 * float accumulation buffer `scratch` of batch*channels*prod(vol_shape) floats
 * (scratch_bytes = that * 4); pass NULL/0 for F32/F64.
 *
 * Workspace of the scatters: with INTERPOL_FLAG_BINNED_SCATTER / INTERPOL_FLAG_AUTO_SCATTER, interpol_push /
 * interpol_count first sort the samples by target brick (push_owner.hip), which needs room for the sorted
 * records (18 B per sample + 4 B per sample and further channel, per brick 1 KiB of run descriptors -- 4 KiB when the items
 * share the target -- and 16 B: run counter, two maxima and the word that marks a brick own_bin's direct scatters wrote under, which the
 * first-writer flush reads, INTERPOL_FLAG_RMW_FLUSH above; that word made the workspace 4 B per brick larger than it was):
 * interpol_scatter_workspace(p, count_only) returns the number of bytes `scratch` must then have
 * (it INCLUDES the fp32 accumulator of a BF16 / F16 target, which comes first), or 0 when the
 * organisation does not apply.  With a smaller (or no) scratch -- or one that is not aligned to 256 bytes (the
 * workspace holds 8- and 16-byte records) -- the operators fall back to the tiled / generic scatters: same results.
 *
 * Round 5: (a) a target SHARED by the batch items (batch stride 0) takes the same organisation -- the items' samples are sorted
 * into ONE brick grid (up to 512 runs per brick) and the bricks flush with plain loads and stores, no atomics; it applies once
 * all items together bring an eighth of a sample per target voxel (BASELINE config 4: 64 sources of 128^3 into 512^3, push + count
 * 16.3 -> 6.3 ms).  (b) Orders 4 and 5 (3-D, F32, private targets with at least a quarter of a sample per voxel):
 * interpol_scatter_workspace returns 16 B per sample + 1 KiB per brick for them and interpol_push / interpol_count -- and the image
 * gradient of interpol_pull_backward, which takes the workspace in its `scratch` -- go through bricks of the target (gather5.hip:
 * scatter5), behind a probe of the call under INTERPOL_FLAG_AUTO_SCATTER (smooth fields keep the LDS tiles): cost independent of
 * the deformation (8 x 1 x 192^3 order 5: 2.9 ms at sigma = 2, 3.1 ms at sigma = 6, where the tiles took 4.2 ms and fell off a cliff).
 * (c) 2-D, per-dim orders 1..3, F32 / BF16 / F16 sources, float32 coordinates (dense grids and displacement fields), private targets
 * with at least a quarter of a sample per pixel: interpol_scatter_workspace returns 16 B per sample + 1 KiB per 32 x 32 brick (plus
 * the accumulator of a 16-bit target) and interpol_push / interpol_count go through bricks of the target (scatter2d.hip) -- always
 * under INTERPOL_FLAG_BINNED_SCATTER, behind a probe of the call under INTERPOL_FLAG_AUTO_SCATTER (the bricks take the call when more than 50
 * pixels per million leave the lean tiles' 64 x 64 boxes AND the samples see a density of at least 0.6 per pixel; a sparser sampling -- a zoom --
 * stays with the tiles, below 0.22 it goes to the generic kernel; smooth fields keep the tiles at +3 %).  BASELINE config 5's shape (32 x 3 x 1024^2 bf16,
 * orders [2, 3]): 1.1 ms at every sigma, where the tiles take 1.04 ms at sigma = 2, 4.3 at 8 and 13.4 at 16.
 *
 * Accuracy of the LDS scatters (every fast path of interpol_push / interpol_count and of the scatter halves of the
 * backward operators; INTERPOL_FLAG_NO_FASTPATH selects the generic kernels, which add floats like the reference's
 * scatter_add_): contributions are summed in FIXED POINT scaled by the largest |source| of the tile / brick they belong
 * to, so the error of a lattice point is ABSOLUTE per tile, not relative to the point's own value.
 *   F32 / BF16 / F16, sample tiles (ops_tiled.hip, ops_tiled2d.hip): each addend rounded to 2^(h-29) of a power of two
 *     >= that maximum, h = the headroom bits the tile's sample density asks for (at most 7);
 *   F32 / BF16 / F16, bricks (push_owner.hip, "magic" format): each addend rounded to nearest at
 *     max|source| * wmax^3 * 2^-22 / 0.999 (wmax = 2/3 cubic, 3/4 quadratic: 2^-23.75 resp. 2^-23.25 of the brick's
 *     maximum), whatever the density; bricks whose stencil counts could overflow 32-bit sums use 64-bit sums of terms
 *     rounded at 2^-30 of a power of two >= the maximum; orders 4 - 5 (gather5.hip: scatter5): the same format in 32-bit
 *     sums, one channel per pass, wmax = 0.599 (order 4) / 0.55 (order 5): 2^-24.2 / 2^-24.6 of the brick's maximum per addend;
 *     2-D (scatter2d.hip): 32-bit sums, each addend rounded to nearest at M * wmax0 * wmax1 / U, M = the largest |source| of the sample
 *     tiles that reach the brick (rounded up to 8 bits), U = min(2^22 * 0.999, 2^31 * 0.99 / n) with n the records of the brick (its
 *     densest cell times the taps when n > 2048): 2^-22 .. 2^-23 of M at one sample per pixel, and never an overflow;
 *   F64 (push_f64.hip): each addend rounded at 2^-51 of a power of two > the tile's maximum -- about 2^-52 of the tile's
 *     largest source per term, again absolute per tile; tiles whose maximum is below 2^-970 use the generic arithmetic.
 * Sums inside a tile / brick are integers: order-free, bit-reproducible.
 * --------------------------------------------------------------------------- */
int64_t interpol_scatter_workspace(const interpol_problem *p, int32_t count_only);
int interpol_pull(const interpol_problem *p, const void *vol, const void *grid, void *val, void *stream);
/* interpol_pull with a workspace (the same seam, interpol/pushpull.py:69-104 -> nd.pull): deformation-independent cost for
 * 3-D quadratic / cubic F32 pulls.  With INTERPOL_FLAG_AUTO_SCATTER the sample tiles (ops_sorted.hip) run first and leave the
 * tiles whose LDS box cannot hold their stencils (more than 512 samples outside it: i.i.d. displacements beyond ~3.5 voxels,
 * folding fields) to a second organisation, which sorts those tiles' samples by the 16^3 brick of the image they read and gathers
 * brick by brick (push_owner.hip: own_bin in index mode + own_gather; 4x2x256^3 cubic, sigma = 6: 9.8 -> 3 ms) -- decided per
 * tile, on the device, no host synchronisation, hipGraph-safe.  INTERPOL_FLAG_BINNED_SCATTER: the bricks for every tile.
 * interpol_pull_workspace(p) returns the bytes `workspace` must have (18 B per sample + 2 KiB per brick + 4 B per tile; 0: the
 * organisation does not apply); with a smaller, missing or not 256-byte aligned workspace the call is interpol_pull.  The
 * workspace need not be cleared.  Same results within float32 rounding (sums in a different order). */
/* Orders 4 and 5 (3-D, float32; round 4, gather5.hip): the same two entry points, interpol_grad_ws and the grid gradient of
 * interpol_pull_backward serve them through bricks of the image of their own (16 B per sample + 1 KiB per brick of workspace).
 * AUTO: order 5 always (8 x 1 x 192^3, sigma = 2: pull 2.57 -> 1.77 ms, grad 2.89 -> 1.96; sigma = 6: 43 -> 1.9 ms), order 4 for
 * grid_grad and the grid gradient, its pull behind a probe of the call (smooth fields stay with the LDS tiles).
 * Orders 6 and 7 (round 6, gather7.hip: bricks of 14^3 cells, always under AUTO): 4 x 2 x 256^3 order 7 pull 14.1 -> 7.2 ms, grid_grad
 * 18.0 -> 8.0; sigma = 6: 167 / 436 -> 7.6 / 8.5 ms; their push / count likewise through scatter5's second compilation: 15.5 -> 11.2 ms,
 * sigma = 6: 250 -> 11.7). */
/* 2-D (round 5, scatter2d.hip: gather2d; per-dim orders 1..3, F32 / BF16 / F16 images, float32 coordinates): interpol_pull_ws, the grid
 * gradient of interpol_pull_backward (grad_vol == NULL for a 16-bit image, whose accumulator owns `scratch`) and both gradients of
 * interpol_push_backward_ws go through 32 x 32 bricks of the image -- 16 B per sample + 1 KiB per brick of workspace -- always under
 * INTERPOL_FLAG_BINNED_SCATTER, behind a probe of the call under INTERPOL_FLAG_AUTO_SCATTER (more than 400 pixels per million outside
 * the lean tiles' boxes and a density of at least 0.6 samples per pixel; sparser samplings -- a zoom beyond ~1.3 whose tiles leave their boxes --
 * go to the generic kernel, as the hand-back of rounds 3 - 4 sent them).  Config 5's shape: pull 0.88 ms at every sigma (tiles: 0.43 at sigma = 2, 2.8 at 8, 3.6 at 16). */
/* Trilinear pulls (round 5; 3-D, order 1 in every dim, F32 with dense grids and displacement fields, BF16 / F16 with dense grids, 32768
 * samples and more; the grid gradient of interpol_pull_backward: F32):
 * interpol_pull_workspace returns 256 -- the verdict of the call's probe (mean absolute second difference of the coordinates above one
 * voxel: rough) is all the workspace holds.  AUTO: rough fields take the class-sorted LDS tiles with K = 1 (4 x 2 x 256^3, i.i.d. noise
 * of sigma = 2: 2.5 -> 1.0 ms), smooth ones the generic kernel, which gathers at the HBM roofline there (0.47 ms); BINNED: the tiles. */
int64_t interpol_pull_workspace(const interpol_problem *p);
int interpol_pull_ws(const interpol_problem *p, const void *vol, const void *grid, void *val, void *workspace, int64_t workspace_bytes, void *stream);
/* grid_grad (interpol_grad) with the same workspace (interpol_pull_workspace(p) bytes; for the grad problem the same number as for
 * the pull of its image): float32, 3-D quadratic / cubic.  INTERPOL_FLAG_BINNED_SCATTER: the bricks of the image always;
 * INTERPOL_FLAG_AUTO_SCATTER: when the probe of the call finds a dense or rough sampling (4 x 2 x 256^3 cubic, sigma = 2: the
 * natural-order tiles 3.5 ms, the bricks ~2.3), the tile / generic kernels otherwise; else, or without a workspace: interpol_grad.
 * Trilinear (float32, 3-D, dense or displacement grids; the 256-byte workspace of the trilinear pull): AUTO -- rough fields take the
 * LDS tiles (sigma = 2: 2.7 -> 1.8 ms), smooth ones the generic kernel (0.7 ms), on the verdict of the pull's probe; BINNED: the tiles. */
int interpol_grad_ws(const interpol_problem *p, const void *vol, const void *grid, void *val, void *workspace, int64_t workspace_bytes, void *stream);
int interpol_push(const interpol_problem *p, const void *val, const void *grid, void *vol,
                  void *scratch, int64_t scratch_bytes, void *stream);
int interpol_count(const interpol_problem *p, const void *grid, void *vol,
                   void *scratch, int64_t scratch_bytes, void *stream);
int interpol_grad(const interpol_problem *p, const void *vol, const void *grid, void *val, void *stream);
int interpol_pushgrad(const interpol_problem *p, const void *val, const void *grid, void *vol,
                      void *scratch, int64_t scratch_bytes, void *stream);
int interpol_hess(const interpol_problem *p, const void *vol, const void *grid, void *val, void *stream);

/* --- fused backward operators -------------------------------------------------
 * interpol_pull_backward  replaces pushpull.grid_pull_backward (pushpull.py:237-258):
 *      grad_vol  (B,C,*in)    += push(grad_out)                 if grad_vol  != NULL
 *      grad_grid (B,*out,D)    = sum_c grad(vol)[c] * grad_out[c] if grad_grid != NULL
 *   no (B,C,N,D) temporary: with both outputs the call runs the push of grad_out and the channel-contracted grid gradient, two passes
 *   over the grid (round 5: the single fused LDS-tile pass is gone -- it was wrong under rough fields; the generic fused kernel remains
 *   for what the tiles decline).
 *   p->val_stride describes grad_out; grad_vol uses p->vol_stride's layout and is
 *   zero-filled here unless INTERPOL_FLAG_ACCUMULATE; grad_grid is contiguous (B,*out,D).
 *   `scratch`: INTERPOL_BF16 / F16 with grad_vol: the float32 accumulator (4 bytes per element of grad_vol).  INTERPOL_F32,
 *   grad_grid alone, 3-D quadratic / cubic, with INTERPOL_FLAG_AUTO_SCATTER or INTERPOL_FLAG_BINNED_SCATTER: optional workspace of
 *   interpol_pull_workspace(p) bytes (256-byte aligned, contents undefined on entry) for the deformation-independent
 *   organisation of the grid gradient -- the samples sorted by the 16^3 brick of the image their stencil starts in, every brick
 *   staged once in LDS (push_owner.hip: own_gather<K, true>).  AUTO: a probe of the call sends dense samplings there altogether
 *   (4 x 2 x 256^3 cubic: 2.0 against 2.4 ms at sigma = 2, 2.9 against 20 at sigma = 6) and expanding ones to the sample tiles,
 *   which then leave the tiles whose stencils do not fit their LDS box to the bricks; BINNED: the bricks always.  Without it
 *   (NULL, too small, misaligned): the sample tiles alone.
 * interpol_push_backward  replaces pushpull.grid_push_backward (pushpull.py:262-282):
 *      grad_val  (B,C,*in)     = pull(grad_vol_out)              if grad_val  != NULL
 *      grad_grid (B,*in,D)     = sum_c grad(grad_vol_out)[c] * val[c] if grad_grid != NULL
 *   p->vol_stride describes grad_vol_out (the incoming gradient, indexed), p->val_stride
 *   describes val; grad_val / grad_grid are contiguous.
 * interpol_count_backward replaces pushpull.grid_count_backward (pushpull.py:286-299):
 *      grad_grid (B,*in,D)     = sum_c grad(grad_vol_out)[c]
 * --------------------------------------------------------------------------- */
int interpol_pull_backward(const interpol_problem *p, const void *grad_out, const void *vol, const void *grid,
                           void *grad_vol, void *grad_grid, void *scratch, int64_t scratch_bytes, void *stream);
int interpol_push_backward(const interpol_problem *p, const void *grad_vol_out, const void *val, const void *grid,
                           void *grad_val, void *grad_grid, void *stream);
int interpol_count_backward(const interpol_problem *p, const void *grad_vol_out, const void *grid,
                            void *grad_grid, void *stream);
/* interpol_push_backward (val != NULL) / interpol_count_backward (val == NULL, grad_val == NULL) with the bricks workspace of the two
 * gathers they consist of -- interpol_pull_workspace(p) bytes, 256-byte aligned, contents undefined on entry; float32, 3-D quadratic /
 * cubic (2-D: see interpol_pull_workspace), INTERPOL_FLAG_AUTO_SCATTER or INTERPOL_FLAG_BINNED_SCATTER: grad_val is the routed pull of grad_vol_out (interpol_pull_ws),
 * grad_grid the routed grid gradient (as interpol_pull_backward's, the roles of the two images swapped: pushpull.py:276-281).
 * Otherwise, or without a workspace: exactly the two calls above. */
int interpol_push_backward_ws(const interpol_problem *p, const void *grad_vol_out, const void *val, const void *grid,
                              void *grad_val, void *grad_grid, void *workspace, int64_t workspace_bytes, void *stream);

/* --- gradient of the matrix of an affine lattice (csrc/affine_grad.hip) ---------------
 * With INTERPOL_FLAG_AFFINE_GRID the coordinates are x(o) = A o + t, so the chain rule through
 * affine_grid (api.py:534-572: matmul + offset) turns the per-sample grid gradient g(b, o) of
 * pushpull.grid_pull_backward (pushpull.py:237-258) / grid_push_backward (262-282) /
 * grid_count_backward (286-299) into
 *      grad_mat[d, e] = sum_b sum_o g_d(b, o) * o_e   (e < D)        grad_mat[d, D] = sum_b sum_o g_d(b, o)
 * with o the integer index of the sample.  g is computed per sample exactly as the generic kernels
 * behind interpol_pull_backward / interpol_push_backward compute it and is never stored: it is summed
 * in DOUBLE (whatever the dtype) in registers, then per wave, per workgroup (LDS) and -- one row of
 * D (D+1) doubles per workgroup in `workspace` -- by a second, single-workgroup kernel in a fixed order.
 * No atomics: the result is bit-identical from run to run.  No host synchronisation: the two launches
 * can be captured into a hipGraph.
 *   interpol_pull_backward_affine : p as for interpol_pull_backward (p->val_stride describes grad_out,
 *       vol with any non-negative strides)
 *   interpol_push_backward_affine : p as for interpol_push_backward (p->vol_stride describes grad_vol_out,
 *       p->val_stride describes val); val == NULL: backward of count (all-ones values)
 *   mat      : the D x (D+1) matrix (what `grid` is in the forward calls)
 *   grad_mat : D x (D+1), row-major, grid_dtype; OVERWRITTEN; summed over the batch (one matrix serves it)
 *   workspace: interpol_affine_backward_workspace(p) bytes (a negative INTERPOL_E_* for an invalid p),
 *       8-byte aligned, contents undefined on entry and on return
 * p->flags must carry INTERPOL_FLAG_AFFINE_GRID (else INTERPOL_E_STRIDE).  Everything is validated before
 * the first launch.  Return value: 0 or a NEGATIVE INTERPOL_E_* only -- a failed launch is
 * INTERPOL_E_LAUNCH, never a positive hipError_t. */
int64_t interpol_affine_backward_workspace(const interpol_problem *p);
int interpol_pull_backward_affine(const interpol_problem *p, const void *grad_out, const void *vol,
                                  const void *mat, void *grad_mat,
                                  void *workspace, int64_t workspace_bytes, void *stream);
int interpol_push_backward_affine(const interpol_problem *p, const void *grad_vol_out,
                                  const void *val /* NULL: count */, const void *mat, void *grad_mat,
                                  void *workspace, int64_t workspace_bytes, void *stream);

/* --- composition of displacement fields (csrc/compose.hip) -----------------------------
 * interpol_compose: out = right + pull(left, id + right) for two voxel displacement fields on one voxel grid --
 *      out[b, o, :] = right[b, o, :] + mask(x) * sum_taps W(x) * sign * left[b, wrap(tap), :],   x = o + right[b, o, :]
 *   what `right + grid_pull(left as a D-channel image, right)` with INTERPOL_FLAG_DISPLACEMENT computes (pushpull.py:35-66
 *   behind add_identity_grid, api.py:490-531; same index, sign, weight and mask rules: one Stencil), in the layout the
 *   fields are stored in: one address computation per tap fetches the D components of `left` in one load, and no
 *   channel-first (B, D, *shape) tensor is written and re-read.  One squaring step of scaling and squaring is
 *   interpol_compose(p, u, u, out).
 * interpol_compose_backward_right: the gradient with respect to `right`,
 *      grad_right[b, o, e] = grad_out[b, o, e] + mask(x) * sum_d grad_out[b, o, d] * d/dx_e pull(left_d)(x)
 *   one pass, no (B, D, *shape, D) Jacobian in memory.  (The gradient with respect to `left` is interpol_push of
 *   grad_out along `right`: a scatter, which keeps its own organisations.)
 * The same interpol_problem: vol_shape / vol_stride describe the lattice of `left` (B, *vol_shape, D), grid_shape /
 * grid_stride describe `right` (B, *grid_shape, D), val_stride describes `out`, `grad_out` and `grad_right`
 * (B, *grid_shape, D); channels = dim (the components); dtype = grid_dtype = INTERPOL_F32 or INTERPOL_F64; flags are
 * ignored (`right` always holds displacements).  The two lattices may differ in shape.
 * Layouts: all tensors point by point and row-major -- component stride 1 (vol_stride[1], grid_stride[4],
 * val_stride[1]), spatial strides those of a dense (*shape, D) array; free batch strides, 0 broadcasts `left` or
 * `right` over the batch (not the output); anything else INTERPOL_E_STRIDE.  Base pointers need the alignment of one
 * element only (4 / 8 bytes).  One item of `left` must span < 4 GiB, like every gather source (INTERPOL_E_SHAPE).
 * Covered: one order 1, 2 or 3 for all dims (order 1 with the weights of iso1.py, as everywhere), every bound and
 * extrapolation mode; other orders INTERPOL_E_ORDER, bf16 / f16 INTERPOL_E_DTYPE -- the caller composes those from
 * interpol_pull.
 * Aliasing: `out` may be `right` (`grad_right` may be `grad_out`): every thread reads its own element before it writes
 * it.  `out` must NOT overlap `left`, which other threads gather from.
 * No workspace, no LDS, no atomics, no state: bit-reproducible, safe under hipGraph capture.  Everything is validated
 * before the launch.  Return value: 0 or a NEGATIVE INTERPOL_E_* only -- a failed launch is INTERPOL_E_LAUNCH. */
int interpol_compose(const interpol_problem *p, const void *left, const void *right, void *out, void *stream);
int interpol_compose_backward_right(const interpol_problem *p, const void *grad_out, const void *left, const void *right,
                                    void *grad_right, void *stream);

/* --- Jacobian of a displacement field at its lattice points (csrc/jacobian.hip) ---------
 * interpol_jacobian: the Jacobian of the transformation id + u of a voxel displacement field u (B, *shape, D) --
 *      J[b, o, d, e] = delta_de + sum_taps (g_e prod_{f != e} w_f)(0) * sign * u[b, wrap(tap), d]
 *   what interpol_grad of u as a D-channel image at the identity grid computes (pushpull.py:146-172, extrapolate = 1), plus
 *   the identity, in the layout the field is stored in.  Row d = component, column e = direction.  The sample points are
 *   the lattice points: the first tap is o - order / 2 and the weights are the order's B-spline and its derivative at
 *   offset 0 (order 1: w = 1, 0 and g = -1, +1, the forward difference u[o + e_e] - u[o]; orders 2, 3: the central
 *   difference along e, smoothed by 1/8, 3/4, 1/8 resp. 1/6, 2/3, 1/6 along the other dims).  Taps whose weight and
 *   derivative weight are both zero are not loaded (the one deviation from interpol_grad: a non-finite value under them
 *   stays without effect).  Index and sign of a tap beyond a face: the bound rules of every other operator.
 *     det_only = 0: out is (B, *shape, D, D), row-major; add_identity = 0 leaves the identity out (the gradient of u).
 *     det_only = 1: out is (B, *shape), det(J) with the identity added whatever add_identity says; expanded along row 0 in
 *                   registers, no matrix is written.
 * interpol_jacdet_backward_field: gfield[b, d, o, e] = grad_out[b, o] * cof(J[b, o])[d][e] (cof = dJ of det = det(J) J^-T),
 *   (B, D, *shape, D): the layout interpol_pushgrad reads.  The gradient of the determinant with respect to u is
 *   interpol_pushgrad of gfield along a zero displacement (INTERPOL_FLAG_DISPLACEMENT), moved to (B, *shape, D).
 *   (The gradient of the matrix itself needs no kernel: interpol_pushgrad of grad_out moved to (B, D, *shape, D).)
 * The same interpol_problem: vol_shape / vol_stride describe u (B, *vol_shape, D); channels = dim (the components); dtype =
 * INTERPOL_F32 or INTERPOL_F64; val_stride[0] is the batch stride of the output (out / gfield), whose items are dense;
 * grad_out is dense (B, *shape).  grid_shape, grid_stride, grid_dtype, extrapolate and flags are ignored.
 * Layouts: u point by point and row-major -- component stride 1 (vol_stride[1]), spatial strides those of a dense
 * (*shape, D) array, a free batch stride >= 0; anything else INTERPOL_E_STRIDE.  Base pointers need the alignment of one
 * element only (4 / 8 bytes).  One item of u must span < 4 GiB, like every gather source (INTERPOL_E_SHAPE).
 * Covered: one order 1, 2 or 3 for all dims, every bound; other orders INTERPOL_E_ORDER, bf16 / f16 INTERPOL_E_DTYPE -- the
 * caller composes those from interpol_grad and interpol_pushgrad.
 * Aliasing: no output may overlap u, which every lattice point gathers from (the caller's check).
 * No workspace, no LDS, no atomics, no state: bit-reproducible, safe under hipGraph capture.  Everything is validated
 * before the launch.  Return value: 0 or a NEGATIVE INTERPOL_E_* only -- a failed launch is INTERPOL_E_LAUNCH. */
int interpol_jacobian(const interpol_problem *p, const void *disp, void *out, int det_only, int add_identity, void *stream);
int interpol_jacdet_backward_field(const interpol_problem *p, const void *grad_out, const void *disp, void *gfield, void *stream);

/* --- smoothness penalty of a displacement field: absolute, membrane, bending (csrc/regulariser.hip) ---------
 * interpol_regulariser: the matrix-vector product L v of a voxel displacement field v (B, *shape, D), in its layout --
 *      (L v)_d = h_d^2 [ absolute v_d + membrane sum_e A_e v_d + bending ( sum_e B_e v_d + sum_{e != f} A_e A_f v_d ) ]
 *      A_e f [o] = (2 f~[o] - f~[o - e] - f~[o + e]) / h_e^2
 *      B_e f [o] = (f~[o - 2e] - 4 f~[o - e] + 6 f~[o] - 4 f~[o + e] + f~[o + 2e]) / h_e^4
 *   with f~[i] = sign(i) f[index(i)] along the axis of the stencil, by the bound rules of every other operator, for every
 *   tap of A_e and B_e (the centre included: dst1 keeps its sign 0 at index 0); A_e A_f is the tensor product of the two
 *   1-D stencils.  The field is in voxels, h = voxel_size (a HOST array of dim doubles, > 0) makes the energy physical.
 * interpol_regulariser_energy: energy[b] = 0.5 sum_o sum_d v_d (L v)_d, (B) in the dtype of the field, without writing L v.
 *   Every product v_d (L v)_d is formed in the field's precision and summed in double, in a fixed order and without
 *   atomics: a constant number of persistent workgroups per batch item, one double each into `workspace`
 *   (interpol_regulariser_energy_workspace(p) bytes, a negative INTERPOL_E_* for an invalid p; it need not be cleared), and
 *   a finishing kernel.  Bit-identical from run to run, and for an item alone or inside a batch.
 * absolute, membrane, bending >= 0 and not all zero, voxel sizes > 0 (else INTERPOL_E_SHAPE); a term whose weight is 0 is
 *   not evaluated (its taps are not loaded).
 * The same interpol_problem as interpol_jacobian: vol_shape / vol_stride describe v (B, *vol_shape, D), point by point and
 * row-major with a free batch stride >= 0 (else INTERPOL_E_STRIDE); channels = dim; dtype = INTERPOL_F32 or INTERPOL_F64
 * (bf16 / f16 INTERPOL_E_DTYPE: the caller computes those in float32); val_stride[0] is the batch stride of `out`, whose
 * items are dense (ignored by the energy); order, grid_*, extrapolate and flags are ignored.  Base pointers need the
 * alignment of one element only.  One item of v must span < 4 GiB (INTERPOL_E_SHAPE).
 * Aliasing: `out` / `energy` / `workspace` must not overlap v, which every lattice point gathers from: INTERPOL_E_STRIDE.
 * No LDS tile, no atomics, no state: safe under hipGraph capture.  Everything is validated before the launch.  Return
 * value: 0 or a NEGATIVE INTERPOL_E_* only -- a failed launch is INTERPOL_E_LAUNCH. */
int interpol_regulariser(const interpol_problem *p, const void *field, void *out, double absolute, double membrane, double bending,
                         const double *voxel_size, void *stream);
int64_t interpol_regulariser_energy_workspace(const interpol_problem *p);
int interpol_regulariser_energy(const interpol_problem *p, const void *field, void *energy, double absolute, double membrane,
                                double bending, const double *voxel_size, void *workspace, int64_t workspace_bytes, void *stream);

/* --- preconditioned conjugate-gradient solve of (H + L) x = g for displacement fields (csrc/regulariser_solve.hip) ---------
 * interpol_regulariser_solve: x (B, *shape, D) after at most max_iter iterations on (H + L) x = g, L the operator of
 *   interpol_regulariser (same weights, voxel sizes and bound rules), H a symmetric positive semi-definite D x D matrix per
 *   lattice point (NOT checked: an indefinite H may give non-finite values, never an access outside the buffers).  Each batch
 *   item runs on its own; inner products are sums of double products in a fixed order, alpha and beta are doubles, rounded to
 *   the field's precision once where they multiply a field:
 *      c_d = h_d^2 [ absolute + membrane sum_e 2 / h_e^2 + bending ( sum_e 6 / h_e^4 + sum_{e != f} 4 / (h_e^2 h_f^2) ) ]
 *      M_o = H_o + diag(c)          (c: the interior diagonal of L; M_o is inverted per point in closed form, never stored)
 *      x = 0;  r = g;  z = M^-1 r;  p = z;  rho = <r,z>;  gamma = <g,g>;  done = (gamma == 0)
 *      for k = 1 .. max_iter, items not done:
 *          q = (H + L) p;   pi = <p,q>;   if pi <= 0 or rho <= 0: done, skip
 *          alpha = rho / pi;  x += alpha p;  r -= alpha q;  z = M^-1 r;  rho' = <r,z>;  sigma = <r,r>;  iterations += 1
 *          if sigma <= tolerance^2 gamma: done
 *          beta = rho' / rho;  rho = rho';  p = z + beta p
 *   A done item is skipped by a uniform branch: its x keeps its bits.  max_iter = 0 writes zeros.
 * gradient: g through the problem's field strides -- the same interpol_problem as interpol_regulariser (vol_shape /
 *   vol_stride: point by point and row-major, a free batch stride >= 0; channels = dim; INTERPOL_F32 or INTERPOL_F64), but
 *   every bound must be one of zero, dct2, dst2, dft, for which L is symmetric (else INTERPOL_E_BOUND).
 * hessian: dense (N, hessian_components) per item with the batch stride hessian_batch_stride (elements; 0 broadcasts one
 *   Hessian to every item).  hessian_components = 0: H = 0, `hessian` may be NULL; = dim: the diagonal; = dim (dim + 1) / 2:
 *   the diagonal first, then the upper triangle row by row ((0,1), (0,2), (1,2) in 3-D); dim = 1: 1 either way.
 * solution: dense (B, *shape, D).  info: NULL, or B x 2 doubles -- (the iterations that changed x, sqrt(sigma / gamma); 0
 *   where gamma = 0 or no iteration ran).  Everything stays on the device: no host synchronisation, no copy; every
 *   iteration is enqueued by this one call (five launches each), so it is safe under hipGraph capture.  No atomics, no
 *   grid-wide barrier, no cooperative launch: bit-identical from run to run, and for an item alone or inside a batch.
 * workspace: interpol_regulariser_solve_workspace(p, hessian_components) bytes (a negative INTERPOL_E_* for an invalid p or
 *   count; a function of p alone), 8-byte aligned, need not be cleared: three fields (r, p and q; z overwrites q in place), the
 *   reduction slots and the scalars of the items.
 * Base pointers of gradient, hessian and solution need the alignment of one element only.
 * Everything is validated before the first launch: INTERPOL_E_DTYPE for a dtype other than float32 / float64;
 *   INTERPOL_E_SHAPE for the shape, the weights, the voxel sizes, hessian_components, a negative max_iter or a negative
 *   tolerance; INTERPOL_E_BOUND; INTERPOL_E_STRIDE for the layout, a negative hessian_batch_stride, a misaligned workspace, and
 *   for a solution, workspace or info that overlaps the gradient, the Hessian or each other; INTERPOL_E_SCRATCH for a
 *   workspace that is too small; INTERPOL_E_NULL for a missing pointer.  Return value: 0 or a NEGATIVE INTERPOL_E_* only -- a
 *   failed launch is INTERPOL_E_LAUNCH. */
int64_t interpol_regulariser_solve_workspace(const interpol_problem *p, int hessian_components);
int interpol_regulariser_solve(const interpol_problem *p, const void *gradient, const void *hessian, int hessian_components,
                               int64_t hessian_batch_stride, void *solution, double absolute, double membrane, double bending,
                               const double *voxel_size, int max_iter, double tolerance, void *info /* B x 2 doubles, may be NULL */,
                               void *workspace, int64_t workspace_bytes, void *stream);

/* --- the sum-of-squares data term of a registration step, fused (csrc/ssd.hip) --------
 * interpol_ssd: loss, gradient and Gauss-Newton Hessian of  1/2 sum_o sum_c weight(o) (moving_c(o + disp(o)) - fixed_c(o))^2  with
 * respect to the voxel displacement field `disp`, in one pass over the samples.  With
 *     w_c(o)  = interpol_pull(moving, disp) under INTERPOL_FLAG_DISPLACEMENT,   G_cd(o) = interpol_grad(...) likewise
 *     r_c     = w_c - fixed_c
 * it writes
 *     loss[b]            = 1/2 sum_o sum_c weight(o) r_c(o)^2                    (B)           no normalisation
 *     gradient[b, o, d]  = weight(o) sum_c r_c(o) G_cd(o)                        (B, *shape, D)
 *     hessian[b, o, k]   = weight(o) sum_c G_cd(o) G_ce(o)                       (B, *shape, K)
 * -- what interpol_regulariser_solve takes as `gradient` and `hessian`.  Out-of-view samples under extrapolate 0 / 2 have w = 0 and
 * G = 0 as in interpol_pull / interpol_grad: r = -fixed, gradient = 0, hessian = 0.  One stencil per sample serves every channel; w
 * and G never reach memory.
 * The problem: vol_* = moving (B, C, *vol_shape), any non-negative strides, as interpol_pull takes its `vol` (one (b, c) image < 4 GiB);
 *   grid_* = disp (B, *grid_shape, D), row-major point by point, free batch stride (INTERPOL_FLAG_DISPLACEMENT is implied; other
 *   coordinate flags are INTERPOL_E_STRIDE); val_* = fixed (B, C, *grid_shape), spatial dims row-major, free batch and channel
 *   strides, as interpol_pull takes its `val`.  A batch stride of 0 broadcasts that input.  dtype = grid_dtype = INTERPOL_F32 or
 *   INTERPOL_F64; dim 1..3; ONE order 1..3 for all dims (else INTERPOL_E_ORDER); every bound; extrapolate 0..2.
 * weight: NULL, or (B, *grid_shape) dense per item with the batch stride weight_batch_stride (elements, >= 0; 0 broadcasts).
 * loss: B elements of the dtype.  gradient: dense (*shape, D) per item, batch stride gradient_batch_stride (elements, >= one item
 *   when batch > 1).  hessian_kind: 0 = no Hessian, `hessian` is ignored; 1 = the diagonal, K = dim; 2 = full, K = dim (dim + 1) / 2,
 *   the diagonal first and then the upper triangle row by row ((0,1), (0,2), (1,2) in 3-D).  hessian: dense (*shape, K) per item,
 *   batch stride hessian_batch_stride.  All base pointers need the alignment of one element only.
 * The loss: weight r_c^2 is formed in the dtype and summed in DOUBLE -- over the channels in the thread, over the workgroup in a
 *   fixed order, one double per workgroup into its own slot of the workspace; a second launch (one workgroup per item) sums an
 *   item's slots in a fixed order.  No atomics; every slot is written, so the workspace need not be cleared; the summation tree of
 *   an item depends on its shape alone: bit-identical from run to run, for an item alone or inside a batch, and under hipGraph replay.
 * workspace: interpol_ssd_workspace(p) bytes (a negative INTERPOL_E_* for an invalid p; a function of p alone), 8-byte aligned.
 * Everything is validated before the first launch: INTERPOL_E_DIM, _ORDER, _BOUND, _DTYPE, _EXTRAP; INTERPOL_E_SHAPE for the extents
 *   and an unknown hessian_kind; INTERPOL_E_STRIDE for the layouts, a negative batch stride, an output batch stride smaller than an
 *   item, a misaligned workspace, and for an output or the workspace that overlaps an input or another output; INTERPOL_E_SCRATCH for
 *   a workspace that is too small; INTERPOL_E_NULL for a missing pointer.  Return value: 0 or a NEGATIVE INTERPOL_E_* only -- a failed
 *   launch is INTERPOL_E_LAUNCH. */
int64_t interpol_ssd_workspace(const interpol_problem *p);
int interpol_ssd(const interpol_problem *p, const void *moving, const void *fixed, const void *disp, const void *weight /* may be NULL */,
                 void *loss, void *gradient, void *hessian, int hessian_kind, int64_t weight_batch_stride,
                 int64_t gradient_batch_stride, int64_t hessian_batch_stride, void *workspace, int64_t workspace_bytes, void *stream);

/* --- the sum-of-squares data term on the matrix of an affine lattice, fused (csrc/ssd_affine.hip) --------
 * interpol_ssd_affine: loss, gradient and Gauss-Newton Hessian of  1/2 sum_o sum_c weight(o) (moving_c(A_b o + t_b) - fixed_c(o))^2
 * with respect to the D (D+1) entries of the matrix [A_b | t_b] of batch item b, in one pass over the samples.  The coordinate of
 * sample o is formed as under INTERPOL_FLAG_AFFINE_GRID (in the dtype: ((A_d0 o_0) + A_d1 o_1 + ..) + t_d with fused
 * multiply-adds), here from ONE MATRIX PER BATCH ITEM.  With o~ = (o_0 .. o_{D-1}, 1), P = D (D+1) and
 *     w_c(o)  = interpol_pull(moving, x),   G_cd(o) = interpol_grad(moving, x),   r_c = w_c - fixed_c
 * it writes
 *     loss[b]                                 = 1/2 sum_o weight(o) sum_c r_c(o)^2                  (B)        no normalisation
 *     gradient[b, d, e]                       = sum_o weight(o) sum_c r_c(o) G_cd(o) o~_e           (B, D, D+1)
 *     hessian[b, d (D+1) + e, d' (D+1) + e']  = sum_o weight(o) sum_c G_cd(o) G_cd'(o) o~_e o~_e'   (B, P, P)  both triangles
 * Out-of-view samples under extrapolate 0 / 2 have w = 0 and G = 0: r = -fixed, no contribution to gradient and Hessian.  Nothing
 * of size N is written: no lattice, no per-sample field.
 * The problem: vol_* = moving (B, C, *vol_shape), any non-negative strides, as interpol_pull takes its `vol` (one (b, c) image < 4 GiB);
 *   grid_shape = the sample lattice, fewer than 2^32 samples (grid_stride is not read; INTERPOL_FLAG_AFFINE_GRID is implied, the
 *   other coordinate flags are INTERPOL_E_STRIDE); val_* = fixed (B, C, *grid_shape), spatial dims row-major, free batch and channel
 *   strides.  A batch stride of 0 broadcasts that input.  dtype = grid_dtype = INTERPOL_F32 or INTERPOL_F64; dim 1..3; ONE order
 *   1..3 for all dims (else INTERPOL_E_ORDER); every bound; extrapolate 0..2; batch <= 65535.
 * mat: (B, D, D+1) of the dtype, each matrix row-major and dense, batch stride mat_batch_stride (elements, >= 0; 0: one matrix for
 *   all).  weight: NULL, or (B, *grid_shape) dense per item with the batch stride weight_batch_stride (elements, >= 0).
 * loss (B), gradient (B, D, D+1) and hessian (B, P, P) are dense, of the dtype; with_hessian: 0 = `hessian` is ignored, 1.  All base
 *   pointers need the alignment of one element only.
 * The sums: per sample the loss term, q_d = weight sum_c r_c G_cd and h_dd' = weight sum_c G_cd G_cd' are formed in the dtype,
 *   converted to double once and accumulated in DOUBLE (73 sums in 3-D, 25 in 2-D, 6 in 1-D; 1 + P without a Hessian) by 1024
 *   persistent workgroups per item, reduced in a fixed order; a second launch (one workgroup per item) sums the workgroups' rows in
 *   a fixed order and rounds once.  No atomics; every row is written, so the workspace need not be cleared; the summation tree of
 *   an item depends on its shape alone: bit-identical from run to run, for an item alone or inside a batch, and under hipGraph replay.
 * workspace: interpol_ssd_affine_workspace(p) bytes (a negative INTERPOL_E_* for an invalid p; a function of p alone), 8-byte aligned.
 * Everything is validated before the first launch: INTERPOL_E_DIM, _ORDER, _BOUND, _DTYPE, _EXTRAP; INTERPOL_E_SHAPE for the extents,
 *   the batch and a with_hessian other than 0 / 1; INTERPOL_E_STRIDE for the layouts, a negative batch stride, a misaligned
 *   workspace, and for an output or the workspace that overlaps an input or another output; INTERPOL_E_SCRATCH for a workspace that
 *   is too small; INTERPOL_E_NULL for a missing pointer.  Return value: 0 or a NEGATIVE INTERPOL_E_* only -- a failed launch is
 *   INTERPOL_E_LAUNCH. */
int64_t interpol_ssd_affine_workspace(const interpol_problem *p);
int interpol_ssd_affine(const interpol_problem *p, const void *moving, const void *fixed, const void *mat, const void *weight /* may be NULL */,
                        void *loss, void *gradient, void *hessian, int with_hessian, int64_t mat_batch_stride,
                        int64_t weight_batch_stride, void *workspace, int64_t workspace_bytes, void *stream);

/* --- the mutual-information data term on the matrix of an affine lattice, fused (csrc/mi_affine.hip) --------
 * interpol_mi_affine: loss, gradient and a majoriser of the Hessian of minus the mutual information between moving(A_b o + t_b) and
 * fixed(o) with respect to the D (D+1) entries of the matrix [A_b | t_b] of batch item b; ONE channel.  The lattice, I = the pull,
 * G = its gradient, the in-view mask m and the layout of gradient and hessian are those of interpol_ssd_affine.  With B = bins,
 * omega = weight m and the five doubles (m_lo, m_sc, f_lo, f_sc, wmax) of item b in `ranges` (converted to the dtype):
 *     t_m = clamp((I - m_lo) m_sc, 0, 1),   u = 1.5 + t_m (B - 4),   taps j = floor(u) - 1 .. floor(u) + 2   (cubic B-spline beta3)
 *     t_f = clamp((fixed - f_lo) f_sc, 0, 1),   k = floor(t_f (B - 1) + 1/2)
 *     P[j, k] = sum_o omega beta3(u - j) [k = k(o)] / W,  W = sum omega;   p_m = sum_k P,  p_f = sum_j P
 *     T[j, k] = log(P / (p_m p_f)) where P > 0, else 0;                    s = (B - 4) m_sc, 0 for a sample whose t_m was clamped
 *     dI = -(omega / W) s sum_j beta3'(u - j) T[j, k],    c = (omega / W) s^2 sum_j |beta3''(u - j)| |T[j, k]|
 * it writes
 *     loss[b]                                 = - sum_jk P T                                        (B)
 *     gradient[b, d, e]                       = sum_o dI G_d o~_e                                   (B, D, D+1)
 *     hessian[b, d (D+1) + e, d' (D+1) + e']  = sum_o c G_d G_d' o~_e o~_e'                         (B, P, P)  both triangles
 *     histogram[b, j, k]                      = P                                                   (B, bins, bins)  NULL: not written
 * Out-of-view samples are excluded (omega = 0).  W <= 0 gives zeros everywhere.  weight >= 0 is assumed, not checked.
 * The problem, mat, weight, loss, gradient, hessian, with_hessian and the batch strides: exactly as for interpol_ssd_affine, with
 *   channels == 1 (else INTERPOL_E_SHAPE).  bins: 8..64 (else INTERPOL_E_SHAPE).  ranges: (B, 5) doubles, dense, 8-byte aligned, on the
 *   device; m_sc = 1 / (m_hi - m_lo) or 0 for a degenerate range, f_sc likewise, wmax = max |weight| of the item (1 without a weight).
 * Precision: the coordinate is formed in the dtype; for the histogram I, u, k and beta3 are evaluated in DOUBLE from the tensors' values
 *   (the weight of a tap at the end of the spline's support has an unbounded relative sensitivity to u, and T reads P relatively); the
 *   per-sample terms of the gradient and of the Hessian are formed in the dtype, as interpol_ssd_affine forms its own.
 * Three stages on `stream`: (1) the histogram in 64-bit fixed point with the quantum q = wmax 2^-min(52, 62 - ceil(log2 N)): LDS
 *   integer adds per workgroup, integer atomics across workgroups into a region of the workspace that a kernel clears first -- exact
 *   in any order; (2) one workgroup per item forms P, the marginals, T and the loss in double and rounds T once to the dtype; (3) the
 *   sums of interpol_ssd_affine with q_d = dI G_d and h_dd' = c G_d G_d', T in LDS, the stencil recomputed, and their finish.
 *   Nothing of size N is written.  No floating-point atomics: bit-identical from run to run, for an item alone or inside a batch,
 *   and under hipGraph replay.
 * workspace: interpol_mi_affine_workspace(p, bins) bytes (a negative INTERPOL_E_* for an invalid p or bins), 8-byte aligned; it need
 *   not be cleared.
 * Everything is validated before the first launch, with the codes of interpol_ssd_affine; `ranges` and `histogram` take part in the
 *   overlap test.  Return value: 0 or a NEGATIVE INTERPOL_E_* only -- a failed launch is INTERPOL_E_LAUNCH. */
int64_t interpol_mi_affine_workspace(const interpol_problem *p, int bins);
int interpol_mi_affine(const interpol_problem *p, const void *moving, const void *fixed, const void *mat, const void *weight /* may be NULL */,
                       const void *ranges, void *loss, void *gradient, void *hessian, void *histogram /* may be NULL */, int with_hessian,
                       int bins, int64_t mat_batch_stride, int64_t weight_batch_stride, void *workspace, int64_t workspace_bytes,
                       void *stream);

/* --- the mutual-information data term on a dense displacement field, fused (csrc/mi.hip) --------
 * interpol_mi: loss, gradient and a per-voxel majoriser of the Hessian of minus the mutual information between moving(o + disp(o))
 * and fixed(o) with respect to the voxel displacement field `disp`; ONE channel.  The lattice, I = the pull, G = its gradient, the
 * in-view mask m and the layout of gradient and hessian are those of interpol_ssd; bins, ranges, t_m, u, the taps, t_f, k, P, p_m,
 * p_f, T, s, dI and c are those of interpol_mi_affine.  It writes
 *     loss[b]             = - sum_jk P T                                        (B)
 *     gradient[b, o, d]   = dI G_d                                              (B, *shape, D)   point by point, gradient_batch_stride
 *     hessian[b, o, k]    = c G_d G_e                                           (B, *shape, K)   hessian_batch_stride
 *     histogram[b, j, k]  = P                                                   (B, bins, bins)  NULL: not written
 *   hessian_kind: 0 none (hessian may be NULL, K = 0), 1 diagonal (K = D), 2 full (K = D (D+1) / 2: the diagonal first, then the upper
 *   triangle row by row) -- what interpol_regulariser_solve takes.
 * Out-of-view samples are excluded from the histogram (omega = 0); their gradient and Hessian are written as zeros.  W <= 0 gives
 *   zeros everywhere; every output is fully written.  weight >= 0 is assumed, not checked.
 * The problem, disp, weight, loss, gradient, hessian, hessian_kind and the batch strides: exactly as for interpol_ssd, with
 *   channels == 1, bins in 8..64 and batch <= 65535 (the item sits on gridDim.y; each INTERPOL_E_SHAPE).  ranges: as for
 *   interpol_mi_affine.
 * Precision: as interpol_mi_affine -- the coordinate in the dtype; for the histogram I, u, k and beta3 in DOUBLE from the tensors'
 *   values; the per-voxel terms in the dtype.
 * Four launches on `stream`, no host synchronisation, capturable: (0) a kernel clears the histogram region of the workspace; (1) the
 *   histogram in 64-bit fixed point with the quantum of interpol_mi_affine, LDS integer adds per workgroup and integer atomics across
 *   workgroups -- exact in any order; (2) one workgroup per item forms P, the marginals, T and the loss in double and rounds T once
 *   to the dtype; (3) one thread per sample recomputes the stencil and stores the two fields, T in LDS.  No floating-point atomics:
 *   bit-identical from run to run, for an item alone or inside a batch, and under hipGraph replay.
 * workspace: interpol_mi_workspace(p, bins) bytes -- two B x bins^2 tables of 8 bytes and 1 / W per item -- (a negative INTERPOL_E_*
 *   for an invalid p or bins), 8-byte aligned; it need not be cleared.
 * Everything is validated before the first launch, in this order: the problem (the codes of interpol_ssd); one channel, the bins and
 *   the batch (INTERPOL_E_SHAPE); hessian_kind (INTERPOL_E_SHAPE), the batch strides (INTERPOL_E_STRIDE), NULL pointers
 *   (INTERPOL_E_NULL), the 8-byte alignment of workspace and ranges (INTERPOL_E_STRIDE), the workspace size (INTERPOL_E_SCRATCH); last
 *   the overlap test over every input and every output, `ranges` and `histogram` included (INTERPOL_E_STRIDE).
 *   Return value: 0 or a NEGATIVE INTERPOL_E_* only -- a failed launch is INTERPOL_E_LAUNCH. */
int64_t interpol_mi_workspace(const interpol_problem *p, int bins);
int interpol_mi(const interpol_problem *p, const void *moving, const void *fixed, const void *disp, const void *weight /* may be NULL */,
                const void *ranges, void *loss, void *gradient, void *hessian /* NULL with hessian_kind 0 */,
                void *histogram /* may be NULL */, int hessian_kind, int bins, int64_t weight_batch_stride,
                int64_t gradient_batch_stride, int64_t hessian_batch_stride, void *workspace, int64_t workspace_bytes, void *stream);

/* --- the local normalised cross-correlation data term of a registration step, fused (csrc/lcc.hip) --------
 * interpol_lcc: loss, gradient and the positive part of the Hessian of the local (windowed) squared correlation coefficient between
 * moving(o + disp(o)) and fixed(o) with respect to the voxel displacement field `disp`.  With I = interpol_pull(moving, disp) and
 * G = interpol_grad(...) under INTERPOL_FLAG_DISPLACEMENT, J = fixed, and per channel
 *     S_X(o) = sum of X over the window |p_d - o_d| <= (window_d - 1) / 2, clipped to the lattice (n(o) points);  X in I, J, I^2, J^2, IJ
 *     cross = S_IJ - S_I S_J / n,  vI = max(S_II - S_I^2 / n, 0),  vJ = max(S_JJ - S_J^2 / n, 0),  den = vI vJ + eps,  cc = cross^2 / den
 *     a = weight 2 cross / den,  c = weight 2 cross^2 vJ / den^2,  f = (a S_J - c S_I) / n;   A, C, F = their sums over the same window
 *     dI = -J A + I C + F
 * it writes
 *     loss[b]            = - sum_o weight(o) sum_c cc_c(o)                       (B)           no normalisation
 *     gradient[b, o, d]  = sum_c dI_c(o) G_cd(o)                                 (B, *shape, D)
 *     hessian[b, o, k]   = sum_c C_c(o) G_cd(o) G_ce(o)                          (B, *shape, K)
 * -- what interpol_regulariser_solve takes as `gradient` and `hessian`.  Out-of-view samples under extrapolate 0 / 2 have I = 0 and
 * G = 0 and enter the window sums as zeros.
 * The problem, weight, loss, gradient, hessian_kind, hessian and the batch strides: exactly as for interpol_ssd.
 * window: `dim` ints, each odd and 1..9 (else INTERPOL_E_SHAPE).  eps: finite and > 0 (else INTERPOL_E_SHAPE).
 * Precision: the coordinate o + disp is formed in the dtype; I is evaluated in double there and rounded to the dtype once; G is formed in
 *   the dtype; the five window sums (the products included), cross, vI, vJ, den, cc, a, c, f and the
 *   loss are formed in DOUBLE from the dtype's I and J (INTERPOL_F64 with windows of up to 5 along the first of three dims, and
 *   every 1-D and 2-D window: in pairs of doubles that carry the rounding errors of the sums, so that S_II - S_I^2 / n does not cancel);
 *   a, c, f stay doubles; A, C, F are summed in double; dI is formed in
 *   double and rounded once; the outputs are in the dtype.
 * Three stages on `stream` (the pull, the statistics, the gradient) and the sum of the loss slots.  No atomics; every slot and every
 *   field of the workspace is written before it is read, so the workspace need not be cleared; every sum runs in an order that
 *   depends on the shape and the window alone: bit-identical from run to run, for an item alone or inside a batch, and under hipGraph
 *   replay.
 * workspace: interpol_lcc_workspace(p) bytes (a negative INTERPOL_E_* for an invalid p; a function of p alone: one double per
 *   workgroup and item, three fields (a, c, f) of batch x channels x samples doubles, then I of as many elements), 8-byte aligned.
 * Everything is validated before the first launch: INTERPOL_E_DIM, _ORDER, _BOUND, _DTYPE, _EXTRAP; INTERPOL_E_SHAPE for the extents,
 *   the window, eps and an unknown hessian_kind; INTERPOL_E_STRIDE for the layouts, a negative batch stride, an output batch stride
 *   smaller than an item, a misaligned workspace, and for an output or the workspace that overlaps an input or another output;
 *   INTERPOL_E_SCRATCH for a workspace that is too small; INTERPOL_E_NULL for a missing pointer.  Return value: 0 or a NEGATIVE
 *   INTERPOL_E_* only -- a failed launch is INTERPOL_E_LAUNCH. */
int64_t interpol_lcc_workspace(const interpol_problem *p);
int interpol_lcc(const interpol_problem *p, const void *moving, const void *fixed, const void *disp, const void *weight /* may be NULL */,
                 void *loss, void *gradient, void *hessian, int hessian_kind, const int *window, double eps,
                 int64_t weight_batch_stride, int64_t gradient_batch_stride, int64_t hessian_batch_stride, void *workspace,
                 int64_t workspace_bytes, void *stream);

/* --- the local normalised cross-correlation data term on the matrix of an affine lattice, fused (csrc/lcc_affine.hip) --------
 * interpol_lcc_affine: the loss of interpol_lcc between moving(A_b o + t_b) and fixed(o), its gradient with respect to the D (D+1)
 * entries of the matrix [A_b | t_b] of batch item b and the positive part of their Hessian.  The coordinate of sample o is formed
 * as by interpol_ssd_affine, from ONE MATRIX PER BATCH ITEM.  With I, G at that coordinate, J, the window sums, a, c, f, A, C, F and
 * dI exactly as interpol_lcc defines them, o~ = (o_0 .. o_{D-1}, 1) and P = D (D+1) it writes
 *     loss[b]                                 = - sum_o weight(o) sum_c cc_c(o)                   (B)        the stages of interpol_lcc
 *     gradient[b, d, e]                       = sum_o sum_c dI_c(o) G_cd(o) o~_e                  (B, D, D+1)
 *     hessian[b, d (D+1) + e, d' (D+1) + e']  = sum_o sum_c C_c(o) G_cd(o) G_cd'(o) o~_e o~_e'    (B, P, P)  both triangles
 * The problem, mat, weight, loss, gradient, hessian, with_hessian and the batch strides: exactly as for interpol_ssd_affine, except
 *   that the batch goes up to 2^31 - 1 (every kernel walks the batch in a loop).  window and eps: as for interpol_lcc.
 * Precision: I, the five window sums, a, c, f, the loss and A, C, F as for interpol_lcc; per sample and channel dI and C are rounded
 *   to the dtype once; G and the products q_d = sum_c dI_c G_cd and h_dd' = sum_c C_c G_cd G_cd' are formed in the dtype, converted
 *   to double once and summed in DOUBLE in a fixed order, as interpol_ssd_affine sums its own.
 * Five stages on `stream`: the pull (writes I), the statistics (a, c, f, the loss slots) and the sum of the slots, a second march
 *   that stores dI and C per sample and channel in the dtype, the sums (1024 persistent workgroups per item; ONE stencil per sample
 *   for all channels) and their finish.  No atomics; everything in the workspace is written before it is read, so the workspace need
 *   not be cleared: bit-identical from run to run, for an item alone or inside a batch, and under hipGraph replay.
 * workspace: interpol_lcc_affine_workspace(p) bytes (a negative INTERPOL_E_* for an invalid p; a function of p alone: the slots and
 *   a, c, f of interpol_lcc, the sums of interpol_ssd_affine, then I and the pairs (dI, C), batch x channels x samples elements
 *   and twice as many), 8-byte aligned.
 * Everything is validated before the first launch, with the codes of interpol_ssd_affine; the window and eps as by interpol_lcc
 *   (INTERPOL_E_SHAPE; a NULL window INTERPOL_E_NULL).  Return value: 0 or a NEGATIVE INTERPOL_E_* only -- a failed launch is
 *   INTERPOL_E_LAUNCH. */
int64_t interpol_lcc_affine_workspace(const interpol_problem *p);
int interpol_lcc_affine(const interpol_problem *p, const void *moving, const void *fixed, const void *mat, const void *weight /* may be NULL */,
                        void *loss, void *gradient, void *hessian, int with_hessian, const int *window, double eps,
                        int64_t mat_batch_stride, int64_t weight_batch_stride, void *workspace, int64_t workspace_bytes, void *stream);

/* --- target-stationary splatting -------------------------------------------------
 * interpol_push_bricks: the same operator as interpol_push (pushpull.py:70-102; with
 * INTERPOL_FLAG_WITH_COUNT also the count image, 106-142), organised for EXPANDING deformations
 * (e.g. 128^3 sources splatted into a shared 512^3 target): the samples are binned by 16^3 target
 * brick (count / scan / fill), every brick is accumulated in LDS by the one workgroup that owns
 * it and stored once, instead of one global atomic per tap.  3-D, INTERPOL_F32 data and grid,
 * channels (+1 with the count) <= 4, batch * samples < 2^32; otherwise INTERPOL_E_DTYPE /
 * INTERPOL_E_DIM / INTERPOL_E_SHAPE and the caller uses interpol_push.  Honours ACCUMULATE,
 * WITH_COUNT, SEPARABLE_GRID, DISPLACEMENT and the shared target (vol batch stride 0).
 * `workspace`: device scratch of interpol_push_bricks_workspace(p) bytes (32 B per sample + 12 B per brick). */
int64_t interpol_push_bricks_workspace(const interpol_problem *p);
int interpol_push_bricks(const interpol_problem *p, const void *val, const void *grid, void *vol,
                         void *workspace, int64_t workspace_bytes, void *stream);

/* --- label maps ------------------------------------------------------------------
 * interpol_pull_labels replaces the per-label loop of api.grid_pull for integer inputs
 * (interpol/api.py:194-205, prefilter=False): vol and val hold int32 LABELS (describe them with
 * dtype = INTERPOL_F32, i.e. 4-byte elements; grid_dtype = INTERPOL_F32); for every sample the
 * label with the largest interpolated indicator value (> 0) under the stencil is returned, the
 * smallest such label on ties, 0 if none -- what the reference's loop over unique() computes,
 * in one pass.  Covered: all dims share one order <= 3 (stencils of up to 64 taps: beyond 27 taps a
 * second kernel visits the distinct labels under the stencil one by one); otherwise INTERPOL_E_ORDER
 * (the caller keeps the loop).  Dense / separable / displacement grids. */
int interpol_pull_labels(const interpol_problem *p, const void *vol, const void *grid, void *val, void *stream);

/* --- separable resampling ------------------------------------------------------
 * interpol_resample_1d: one pass of a tensor-product resampling -- what `resize` / `restrict`
 * (interpol/resize.py:13-119, restrict.py:9-121) compute through grid_pull / grid_push on
 * `stack(meshgrid_ij(*lin), -1)`, factorised into D one-dimensional passes (K+1 taps per
 * output instead of (K+1)^D; no grid tensor).  Contiguous (outer, n, inner) arrays.
 *   adjoint == 0 : src (outer, n_lattice, inner), lin[n_samples] -> dst (outer, n_samples, inner)
 *                  dst[b,s,c] = mask(lin[s]) * sum_j w_j sign_j src[b, wrap(i0+j), c]
 *   adjoint == 1 : src (outer, n_samples, inner) -> dst (outer, n_lattice, inner); the exact adjoint of the above (f32 / f64 only).
 *                  Round 5: with n_samples <= 4096 and inner == 1 or inner >= 64 it is a GATHER -- for a non-decreasing `lin` the samples
 *                  whose stencil covers a lattice point are a contiguous range (bisection), the samples that leave the lattice come back
 *                  through the boundary condition and are visited by every output; an unsorted `lin` is detected on the device and served by
 *                  visiting every sample: no atomics, every element of dst written once, bit-reproducible.  Otherwise dst is zero-filled
 *                  here and the taps are added with float atomics.
 * `mode`: 0 nd, 1 iso1, 2 iso0 semantics -- decided by ALL dims of the D-dimensional
 * operator (pushpull.py:48-66), so the caller passes it.  lin is float32 (float64 for F64
 * data).  n_lattice * inner * sizeof(element) must be < 4 GiB, n_samples * inner < 2^32. */
int interpol_resample_1d(int32_t dtype, int32_t lin_dtype, int32_t order, int32_t bound, int32_t extrapolate, int32_t mode,
                         int32_t adjoint, int64_t outer, int64_t n_samples, int64_t n_lattice, int64_t inner,
                         const void *src, const void *lin, void *dst, void *stream);
/* 1 when interpol_resample_1d(adjoint = 1) serves (dtype, n_samples, inner) with the gathering kernel (no atomics, no zero-fill), else 0:
 * the ONE statement of that rule -- the host layer (interpol/separable.py) asks instead of repeating it. */
int32_t interpol_resample_1d_gathers(int32_t dtype, int64_t n_samples, int64_t inner);

/* --- prefilter -----------------------------------------------------------------
 * interpol_spline_filter replaces coeff.spline_coeff (interpol/coeff.py:288-313,
 * filter coeff.py:258-284): in-place interpolating-coefficient IIR along the
 * middle axis of a contiguous (outer, n, inner) array.  order 0/1 = no-op.
 * bound codes as above; dst1/dst2 return INTERPOL_E_PREFILTER (coeff.py:243-244).
 * --------------------------------------------------------------------------- */
int interpol_spline_filter(void *data, int32_t dtype, int64_t outer, int64_t n, int64_t inner,
                           int32_t bound, int32_t order, void *stream);
/* The same filter reading `src` and writing `data` (same layout, no overlap unless src == data): the
 * first filtered dimension of an out-of-place spline_coeff_nd (coeff.py:317-347) then costs one read
 * and one write instead of a copy followed by an in-place pass. */
int interpol_spline_filter_to(const void *src, void *data, int32_t dtype, int64_t outer, int64_t n, int64_t inner,
                              int32_t bound, int32_t order, void *stream);

/* --- host-side helpers (no GPU needed) ------------------------------------------
 * The exact scalar primitives the kernels use, compiled for the host so they
 * can be checked without a device:
 *   interpol_host_bound_index / _sign  = Bound.index / Bound.transform (bounds.py:30-89);
 *                                        sign returns 2 where the reference returns None
 *   interpol_host_weight(order, x, which) which = 0 fastweight, 1 fastgrad, 2 fasthess
 *                                        (splines.py:30-195)
 * --------------------------------------------------------------------------- */
int32_t interpol_host_bound_index(int32_t bound, int32_t i, int32_t n);
int32_t interpol_host_bound_sign(int32_t bound, int32_t i, int32_t n);
double  interpol_host_weight(int32_t order, double x, int32_t which);
float   interpol_host_weight_f32(int32_t order, float x, int32_t which);

/* --- the tile hand-back (csrc/defer.hip; the library's state: "Conventions" above) --
 * The LDS-tiled kernels hand tiles whose stencils do not fit their LDS box back to the generic kernel of the same
 * operator, launched right behind them on the same stream.  The two kernel families sum in different orders, so
 * WHETHER a launch hands back shows in the last bits of the result:
 *   INTERPOL_HANDBACK_ADAPTIVE (default): a stream hands back only after one of its recent launches met such a
 *       tile (a flag the kernels store into pinned host memory, read without synchronisation at the next launch):
 *       smooth workloads never pay the second kernel, but a result can depend on the history of the stream;
 *   INTERPOL_HANDBACK_ALWAYS / _NEVER: every launch / no launch hands back: each operator is then a deterministic
 *       function of its inputs, as the reference's gather is (nd.py:118-136).
 * Round 5: the hand-back only exists where no device-side router does.  Calls that carry a workspace for the bricks --
 * interpol_push / interpol_count with INTERPOL_FLAG_AUTO_SCATTER or _BINNED_SCATTER, interpol_pull_ws, interpol_grad_ws,
 * interpol_pull_backward / interpol_push_backward_ws with the bricks' workspace (3-D orders 2 - 7 and mixed 1 - 3, 2-D orders 1 - 3, as each
 * entry point documents) -- never hand back: their organisation is chosen by a probe of THIS call's coordinates, so the result is a
 * function of the inputs under every mode (tests: test_routed_operators_do_not_depend_on_the_streams_history).  The modes
 * below still govern 3-D order 1, orders 6 - 7, 2-D grid_grad (a generic kernel) and every call without a workspace.
 * interpol_set_handback(mode) returns the previous mode (process-wide; the environment variable
 * INTERPOL_HANDBACK = adaptive | always | never sets the initial one).
 * interpol_release_stream(stream): the hand-back slot (3 MiB of device memory) of `stream` on the current device goes
 * back to the pool; call it before destroying a stream that ran stretched workloads (optional: slots are recycled
 * least-recently-used).  Returns 1 when the stream held a slot.  Thread-safe, like every entry point: launches of
 * several host threads on one stream are serialised per stream. */
#define INTERPOL_HANDBACK_ADAPTIVE 0
#define INTERPOL_HANDBACK_ALWAYS   1
#define INTERPOL_HANDBACK_NEVER    2
int32_t interpol_set_handback(int32_t mode);
int32_t interpol_release_stream(void *stream);

/* --- the linear-elastic member of the smoothness penalty, and sliding boundaries (csrc/regulariser*.hip) ---------
 * The operator of interpol_regulariser with two more non-negative weights, shears (mu) and div (lambda) -- the penalty on the
 * symmetric part of the Jacobian and on the divergence of u_c = h_c v_c, discretised as SPM does:
 *      (L v)_c += h_c^2 [ shears sum_e A_e v_c + (shears + div) A_c v_c ]  -  (shears + div) sum_{e != c} X_ce v_e
 *      X_ce f [o] = ( f~[o + c + e] - f~[o + c - e] - f~[o - c + e] + f~[o - c - e] ) / 4          (no voxel size: h_c h_e cancels)
 *   f~ is the component extended axis by axis by the bound rules (the diagonal taps are tensor products).  With bending the
 *   diagonal points are those of the mixed terms and are loaded once; with membrane alone the stencil has 7 + 12 = 19 points in 3-D.
 * weights: a HOST array of five doubles -- absolute, membrane, bending, shears, div; each finite and >= 0, not all zero
 *   (else INTERPOL_E_SHAPE).
 * Bounds: the codes 0..6 of every entry point, and INTERPOL_BOUND_SLIDING, which ONLY these entry points take: in a sliding
 *   dimension d, component d of the field is extended by dst2 along d and every other component by dct2 (one index map; the
 *   sign flips on reflected taps of component d).  It applies to every term.
 * Symmetry: L is symmetric positive semi-definite when every dimension is zero, dft or sliding; without elastic weights also
 *   dct2 and dst2.  interpol_regulariser_elastic and _energy evaluate L under every bound; interpol_regulariser_elastic_solve
 *   answers INTERPOL_E_BOUND where L is not symmetric.  Its preconditioner grows by
 *      c_d += h_d^2 [ shears sum_e 2 / h_e^2 + (shears + div) 2 / h_d^2 ]
 * Everything else -- the problem, the layouts, the workspaces (the same sizes; the _workspace queries below accept
 *   INTERPOL_BOUND_SLIDING), aliasing, validation before the first launch, return values, determinism -- is that of
 *   interpol_regulariser, interpol_regulariser_energy and interpol_regulariser_solve.  With shears = div = 0 and no sliding
 *   dimension the results are theirs bit for bit. */
#define INTERPOL_BOUND_SLIDING 7
int interpol_regulariser_elastic(const interpol_problem *p, const void *field, void *out, const double *weights /* 5, host */,
                                 const double *voxel_size, void *stream);
int64_t interpol_regulariser_elastic_energy_workspace(const interpol_problem *p);
int interpol_regulariser_elastic_energy(const interpol_problem *p, const void *field, void *energy, const double *weights /* 5, host */,
                                        const double *voxel_size, void *workspace, int64_t workspace_bytes, void *stream);
int64_t interpol_regulariser_elastic_solve_workspace(const interpol_problem *p, int hessian_components);
int interpol_regulariser_elastic_solve(const interpol_problem *p, const void *gradient, const void *hessian, int hessian_components,
                                       int64_t hessian_batch_stride, void *solution, const double *weights /* 5, host */,
                                       const double *voxel_size, int max_iter, double tolerance,
                                       void *info /* B x 2 doubles, may be NULL */, void *workspace, int64_t workspace_bytes, void *stream);

/* --- multigrid preconditioner for the solve of (H + L) x = g (csrc/regulariser_multigrid.hip) ---------
 * interpol_regulariser_multigrid_solve: the conjugate gradients of interpol_regulariser_elastic_solve -- the same problem, five
 *   host weights, bounds (zero, dft, INTERPOL_BOUND_SLIDING; without shears and div also dct2, dst2), Hessian layouts, info,
 *   guards and stopping test -- with z = V(r), one multigrid V-cycle, in the place of z = M^-1 r:
 *      levels: level 0 is the lattice; dimension d is halved iff n_d is even and n_d / 2 >= 4, else kept (semi-coarsening); the
 *        last level is the one on which nothing can be halved.  s_d = 2 where halved, else 1; h_{l+1,d} = s_d h_{l,d};
 *        kappa_{l+1} = kappa_l prod_d s_d, kappa_0 = 1
 *      A_l = H_l + L(kappa_l weights, h_l, bound);  M_l = H_l + diag(c(kappa_l weights, h_l)), inverted per point in closed form
 *      P_l (coarse -> fine, per component c): along each halved dimension fine i = 3/4 e[i >> 1] + 1/4 e[(i >> 1) -+ 1] (minus
 *        for even i), an out-of-range coarse index extended by the bound of that dimension for that component (dft wraps, dct2
 *        reflects, dst2 reflects with a sign flip, zero gives 0, sliding: dst2 for c = d and dct2 otherwise); times s_c
 *      restriction = P_l^T, as a gather: coarse j sums fine 2j-1 .. 2j+2 with 1/4, 3/4, 3/4, 1/4, the same extension; times s_c
 *      H_{l+1}[o] = S (sum over the children of o of H_l) S, S = diag(s); built once per call
 *      V(l, r): x = 0; nu sweeps x <- x + 1/2 M_l^-1 (r - A_l x) (nu = smoothing; 8 on the last level, which returns x);
 *               d = r - A_l x;  x <- x + P_l V(l + 1, P_l^T d);  nu more sweeps
 *   smoothing: 1..1024 (else INTERPOL_E_SHAPE).  A lattice that cannot be coarsened has one level (8 sweeps).
 *   Every kernel is a gather without atomics; the whole cycle is enqueued by the one call inside the loop, nothing synchronises
 *   with the host (safe under hipGraph capture); bit-identical from run to run and for an item alone or inside a batch.  An
 *   item that is done is skipped by every pass of the cycle as well (a uniform branch): its x keeps its bits.
 * interpol_regulariser_multigrid_cycle: out (B, *shape, D), dense = V(residual) alone; `residual` through the problem's field
 *   strides, like `gradient`.
 * workspace: interpol_regulariser_multigrid_solve_workspace / _cycle_workspace(p, hessian_components) bytes (a negative
 *   INTERPOL_E_* for an invalid p or count; a function of p alone), 8-byte aligned, need not be cleared.  Solve: five fields of
 *   level 0 (r, p, q, the sweep buffer a_0 and z = b_0), the reduction slots, the scalars of the items; then for every level
 *   l >= 1 its right-hand side r_l, its two sweep buffers a_l and b_l (x_l ping-pongs between them; d_l = r_l - A_l x_l is
 *   written to the idle one) and H_l of the Hessian pyramid.  Cycle: a_0 and the levels l >= 1 (b_0 is `out`).
 * Validation before the first launch, alignment, aliasing (out / solution, workspace, info against the inputs and each other)
 *   and return values: those of interpol_regulariser_solve. */
int64_t interpol_regulariser_multigrid_solve_workspace(const interpol_problem *p, int hessian_components);
int interpol_regulariser_multigrid_solve(const interpol_problem *p, const void *gradient, const void *hessian, int hessian_components,
                                         int64_t hessian_batch_stride, void *solution, const double *weights /* 5, host */,
                                         const double *voxel_size, int smoothing, int max_iter, double tolerance,
                                         void *info /* B x 2 doubles, may be NULL */, void *workspace, int64_t workspace_bytes, void *stream);
int64_t interpol_regulariser_multigrid_cycle_workspace(const interpol_problem *p, int hessian_components);
int interpol_regulariser_multigrid_cycle(const interpol_problem *p, const void *residual, const void *hessian, int hessian_components,
                                         int64_t hessian_batch_stride, void *out, const double *weights /* 5, host */,
                                         const double *voxel_size, int smoothing, void *workspace, int64_t workspace_bytes, void *stream);

int32_t     interpol_abi_version(void);
/* 1 for a library built with the measured-slower experimental organisations (torch-interpol_amd/experiments/, `make
 * experiments`: INTERPOL_FLAG_SMALL_TILES and debug bit 4096 select them); 0 for the product library, which ignores both. */
int32_t     interpol_has_experiments(void);
const char *interpol_error_string(int code);
/* name of the kernel family the dispatcher would pick for `p` and op
 * ("pull","push","count","grad","pushgrad","hess"); for tests and profiling. */
const char *interpol_kernel_name(const interpol_problem *p, const char *op);

#ifdef __cplusplus
}
#endif
#endif /* INTERPOL_HIP_H */
