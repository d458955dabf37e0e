"""Backend switch kept for drop-in compatibility with the reference
(`interpol/backend.py:1`).  The external `jitfields` package is not part of this
build; setting the flag makes the API raise instead of silently ignoring it."""
jitfields = False

# Scatter operators (grid_push / grid_count and the scatter halves of the backward passes) accumulate
# tile by tile in LDS in FIXED POINT scaled by the tile's largest |source| (csrc/ops_tiled.hip): every
# contribution is rounded to about 2.5e-6 of that maximum at worst -- far below float32 rounding of the
# sums for ordinary images, but an ABSOLUTE error per tile: in a tile that holds both a spike and values
# many orders of magnitude smaller, the small voxels lose significant digits (the reference accumulates
# in float, relative to the local sum).  Set `exact_scatter = True` (or INTERPOL_EXACT_SCATTER=1 in the
# environment) to route every scatter through the generic kernels, which use float atomics like the
# reference's scatter_add_ -- two orders of magnitude slower at BASELINE config 2.
exact_scatter = False

# grid_push / grid_count: two organisations of the same scatter (same results within float32 rounding).  Times: 4x2x256^3 cubic
# dct2 on one MI355X, round 5 (HISTORY.md 4.2c, profiles/r05_rough_rows.txt).
#   * sample-stationary tiles (csrc/ops_tiled.hip): 16^3 tiles of samples accumulate in an LDS box that their
#     stencils must fit (33 x 33 x 32 lattice points); fastest for smooth deformations (2.2 ms at the identity,
#     3.5 ms under i.i.d. displacements of sigma = 2 voxels) and sharply slower beyond that (sigma = 3 / 4 / 6:
#     4.9 / 8.5 / 127 ms);
#   * owner-computes bricks (csrc/push_owner.hip): the samples are first sorted by target brick; cost nearly independent
#     of the deformation (2.8 - 3.6 ms from the identity to sigma = 6), about 22 bytes of workspace per sample point.
# `rough_deformations = None` (default): a probe kernel inside every call examines 128 tiles of the sample grid and
# gates the two organisations on the device (no host synchronisation, stateless, hipGraph-safe; ~50 us).
# Memory: under the default (and under True) every 3-D quadratic / cubic grid_push / grid_count -- and the image gradient of
# grid_pull's backward, which is such a push -- uses the bricks' workspace: about 22 bytes per sample point plus 1 KiB per 16^3 brick
# of the target (1.7 GB at 4x2x256^3), whichever organisation the probe then picks.  One buffer per (device, stream, host thread) is
# kept between calls and grown on demand, at most four of them (`release_workspaces()` frees them); it is only taken when it fits comfortably (at most half of
# the memory that is available), else the call falls back to the tiles, which need none (interpol/_hip.py: _optional_workspace).
# grid_pull (3-D quadratic / cubic, float32) is routed too, per TILE: the sample tiles of csrc/ops_sorted.hip leave the tiles whose
# LDS box cannot hold their stencils to bricks of the IMAGE (csrc/push_owner.hip: own_gather; 18 bytes of workspace per sample,
# allocated per call like the push's): 4x2x256^3 cubic under i.i.d. noise of sigma = 6 voxels 9.8 -> 3 ms; ~3 % on smooth fields.
# grid_grad, the grid gradient of grid_pull's backward and both gradients of grid_push's / grid_count's backward (float32, 3-D
# quadratic / cubic) take the same bricks: dense samplings altogether (a probe of the call), expanding ones stay with the tiles.
# True: always the bricks.  False: always the tiles (no workspace is allocated).
# Reproducibility: the organisation -- hence the summation order, hence the last bits of a result -- may differ between the
# settings and, under None, between calls whose probes decide differently; every organisation is held to the same tolerance
# (1e-5 of max|ref|).  Under None / True the backward of grid_pull is two passes (image gradient = grid_push of grad_out through
# this router, then the grid gradient), not the fused kernel.
rough_deformations = None

# interpol.compose / interpol.exp: the spline orders whose composition runs the fused point-by-point kernel (csrc/compose.hip; GPU,
# D <= 3, float32 / float64); every other order is composed from grid_pull, whose LDS-tiled and brick organisations win once the
# stencil has 27 or 64 taps (1 x 256^3 x 3, profiles/compose.txt).  The library instantiates orders 1, 2 and 3: (1, 2, 3) sends
# them all to the fused kernel (tests, timing).
fused_compose_orders = (1,)

# interpol.jacobian / interpol.jacdet: the spline orders whose Jacobian runs the fused lattice-point kernels (csrc/jacobian.hip; GPU,
# D <= 3, float32 / float64); every other order is composed from grid_grad at a zero displacement (and grid_pushgrad backward).  An
# order is listed when its fused forward and forward + backward both beat the composed route on smooth and on i.i.d. fields at
# 1 x 256^3 x 3 (profiles/jacobian.txt).  The library instantiates orders 1, 2 and 3 whatever is listed here (tests, timing).
fused_jacobian_orders = (1, 2, 3)

# interpol.regulariser / interpol.regulariser_energy: True runs the fused lattice-point kernels (csrc/regulariser.hip; GPU, D <= 3,
# float32 / float64), False the composed form (interpol/torch_kernels.py: one index_select pass per tap), which also serves
# everything the kernels do not cover.  The library builds the kernels either way (tests, timing).  Measured at 1 x 256^3 x 3 and
# 32 x 1024^2 x 2: profiles/regulariser.txt.
fused_regulariser = True

# interpol.regulariser_solve: True runs the fused conjugate-gradient kernels (csrc/regulariser_solve.hip; GPU, D <= 3, float32 /
# float64: every iteration enqueued from one C call, alpha, beta and the stopping test on the device), False the composed form
# (interpol/torch_kernels.py: the same algorithm around `ops.regulariser`, element-wise passes and torch.where masks), which
# also serves everything the kernels do not cover.  The library builds the kernels either way (tests, timing).  Measured at
# 1 x 256^3 x 3 and 32 x 1024^2 x 2: profiles/regulariser_solve.txt.
fused_regulariser_solve = True

# interpol.regulariser_solve(preconditioner='multigrid'): True (default) runs the fused V-cycle and its conjugate gradients
# (csrc/regulariser_multigrid.hip; GPU, D <= 3, float32 / float64); False routes every such call to the composed form
# (interpol/torch_kernels.py: the same cycle around `ops.regulariser`, index_select grid transfers), which also serves
# everything the kernels do not cover.  Measured at 1 x 256^3 x 3 and 32 x 1024^2 x 2: profiles/multigrid.txt.
fused_regulariser_multigrid = True

# interpol.ssd_gauss_newton: the spline orders whose data term runs the fused kernel (csrc/ssd.hip; GPU, D <= 3, float32 / float64,
# one order for all dims); every other order -- and everything the kernel does not cover -- runs the composed form
# (interpol/torch_kernels.py: grid_pull, grid_grad and element-wise passes).  An order is listed when the fused kernel beats the
# composed form on both the smooth and the i.i.d. sigma = 2 field at 1 x 1 x 256^3, 1 x 3 x 256^3 and 32 x 1 x 1024^2 float32
# (profiles/ssd.txt): order 1 by 2.5 - 8.4 x, order 2 by 1.16 - 5.5 x.  Order 3 wins on smooth fields (2.7 - 4.6 x) and in 2-D, and
# loses on the rough 3-D field with three channels (6.8 against 4.5 ms: 64 scattered taps per channel and sample, where grid_pull /
# grid_grad have their class-sorted tiles and bricks), so it stays composed.  `hessian=None` has a list of its own, applied on top:
# without the six Hessian passes the composed form is a pull, a grad and four element-wise passes, and only order 1 beats it on
# both fields (order 2: 2.3 x smooth, 0.99 x rough; order 3: 1.6 x, 0.60 x).  () switches the fused kernel off.  The library
# instantiates orders 1, 2 and 3 whatever is listed here (tests, timing).
fused_ssd_orders = (1, 2)
fused_ssd_orders_without_hessian = (1,)

# interpol.ssd_gauss_newton_affine: the spline orders whose data term runs the fused kernel (csrc/ssd_affine.hip; GPU, D <= 3,
# float32 / float64, one order for all dims); every other order -- and everything the kernel does not cover -- runs the composed
# form (interpol/torch_kernels.py: a dense lattice per item, `ops.ssd_gauss_newton` and the contraction of its nine fields with
# the index moments).  An order is listed when the fused kernel beats the composed form at every measured shape
# (profiles/ssd_affine.txt: 1 x 1 x 256^3 with and without the Hessian, 4 x 2 x 256^3 cubic, 32 x 1 x 1024^2; float32).  All
# three do, by 86 - 3600 x: 0.63 / 0.85 / 1.24 ms against 2276 - 2280 at 256^3 with the Hessian, 0.25 / 0.43 / 0.84 against
# 471 - 474 without, 7.32 against 2290 at 4 x 2 x 256^3 cubic, 0.53 / 0.54 / 0.71 against 58.7 - 60.9 at 32 x 1024^2 (the composed
# form is two float64 skinny GEMMs).
# () switches the fused kernel off.  The library instantiates orders 1, 2 and 3 whatever is listed here (tests, timing).
fused_ssd_affine_orders = (1, 2, 3)

# interpol.mi_gauss_newton_affine: the spline orders whose data term runs the fused kernels (csrc/mi_affine.hip; GPU, D <= 3, float32 /
# float64, one channel, one order for all dims, 8 <= bins <= 64); every other order -- and everything the kernels do not cover --
# runs the composed form (interpol/torch_kernels.py: a dense lattice per item, grid_pull, grid_grad, `index_add_` into a float64
# histogram and two float64 contractions).  The rule of `fused_ssd_affine_orders`: an order is listed when the fused route beats
# the composed form at every measured shape (tools/time_mi_affine.py, profiles/mi_affine.txt: 1 x 1 x 256^3 at 32 and 64 bins, with and
# without the Hessian, 4 x 1 x 256^3 cubic, 32 x 1 x 1024^2; float32).  All three do, by 770 - 13900 x: 1.15 / 1.54 / 2.15 ms against
# 11870 - 12729 at 256^3 and 32 bins with the Hessian, 16.4 against 34124 at 4 x 1 x 256^3 cubic, 1.31 / 1.37 / 1.55 against 1029 - 1334
# at 32 x 1024^2 (the composed form is `index_add_` with floating atomics into a few hundred bins).  () switches the fused kernels
# off.  The library instantiates orders 1, 2 and 3 whatever is listed here (tests, timing).
fused_mi_affine_orders = (1, 2, 3)

# interpol.mi_gauss_newton: the spline orders whose data term runs the fused kernels (csrc/mi.hip; GPU, D <= 3, float32 / float64,
# one channel, one order for all dims, 8 <= bins <= 64); every other order -- and everything the kernels do not cover -- runs the
# composed form (interpol/torch_kernels.py: grid_pull, grid_grad at a displacement, `index_add_` into a float64 histogram and
# element-wise passes).  The rule of `fused_mi_affine_orders`: an order is listed when the fused route beats the composed form on
# both the smooth and the i.i.d. sigma = 2 field at every measured shape (tools/time_mi.py, profiles/mi.txt: 1 x 1 x 256^3 at 32
# and 64 bins, with and without the Hessian, 32 x 1 x 1024^2; float32).  All three do, by 660 - 13300 x: 0.81 / 1.32 / 1.84 ms on the
# smooth and 1.14 / 2.17 / 3.73 ms on the rough field against 9837 - 10828 at 256^3 and 32 bins with the Hessian, 1.25 / 1.32 / 1.45 and
# 1.28 / 1.50 / 1.90 against 1003 - 1401 at 32 x 1024^2 (the composed form is `index_add_` with floating atomics into a few hundred bins).
# () switches the fused kernels off.  The library instantiates orders 1, 2 and 3 whatever is listed here (tests, timing).
fused_mi_orders = (1, 2, 3)

# interpol.lcc_gauss_newton: the spline orders whose data term runs the fused kernels (csrc/lcc.hip; GPU, D <= 3, float32 / float64,
# one order for all dims, odd windows up to 9); every other order -- and everything the kernels do not cover -- runs the composed
# form (interpol/torch_kernels.py: grid_pull, grid_grad, eight separable window sums in float64 and element-wise passes).  The rule
# of `fused_ssd_orders`: an order is listed when the fused route beats the composed form on both the smooth and the i.i.d.
# sigma = 2 field at every measured shape (tools/time_lcc.py, profiles/lcc.txt: 1 x 1 x 256^3 at windows 5 and 9, 1 x 3 x 256^3 and
# 32 x 1 x 1024^2 at window 9, float32).  All three orders do: order 1 by 5.0 - 13.0 x, order 2 by 3.8 - 12.6 x, order 3 by
# 2.8 - 10.8 x (the smallest margin: 1 x 3 x 256^3, rough, cubic, 20.7 against 58.3 ms).  () switches the fused kernels off.  The
# library instantiates orders 1, 2 and 3 whatever is listed here (tests, timing).
fused_lcc_orders = (1, 2, 3)

# interpol.lcc_gauss_newton_affine: the spline orders whose data term runs the fused kernels (csrc/lcc_affine.hip; GPU, D <= 3,
# float32 / float64, one order for all dims, odd windows up to 9); every other order -- and everything the kernels do not cover --
# runs the composed form (interpol/torch_kernels.py: a dense lattice per item, `ops.lcc_gauss_newton` -- itself the fused dense
# term -- and the contraction of its nine fields with the index moments).  The rule of `fused_ssd_affine_orders`: an order is listed
# when the fused route beats the composed form at every measured shape (tools/time_lcc_affine.py, profiles/lcc_affine.txt:
# 1 x 1 x 256^3 at windows 5 and 9 with and without the Hessian, 4 x 1 x 256^3 cubic, 32 x 1 x 1024^2; float32).
# All three do, by 21 - 1320 x: 1.72 / 2.54 / 2.77 ms against 2274 - 2276 at 256^3 and window 5 with the Hessian, 3.19 / 4.01 / 4.27
# against 2276 - 2278 at window 9, 1.33 - 4.05 against 471 - 476 without the Hessian, 16.7 against 2285 at 4 x 1 x 256^3 cubic, 2.19 / 2.25 /
# 2.91 against 60.8 - 61.3 at 32 x 1024^2 (the composed form is two float64 skinny GEMMs behind the 1.4 - 4.5 ms of the dense term).
# () switches the fused kernels off.  The library instantiates orders 1, 2 and 3 whatever is listed here (tests, timing).
fused_lcc_affine_orders = (1, 2, 3)


def release_workspaces():
    """The routed organisations keep ONE workspace per (device, stream, host thread) between calls (interpol/_hip.py:
    _optional_workspace; 1.7 GB at 4x2x256^3 once a push has run, shared by pull / push / backward; at most four are kept): this
    gives them back to torch's allocator -- call it next to torch.cuda.empty_cache()."""
    from . import _hip
    _hip.release_workspaces()


def want_exact_scatter():
    import os
    return bool(exact_scatter) or os.environ.get("INTERPOL_EXACT_SCATTER", "0") not in ("", "0")
