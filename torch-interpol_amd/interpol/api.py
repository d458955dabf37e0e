"""Public API: `grid_pull / grid_push / grid_count / grid_grad / spline_coeff /
spline_coeff_nd` with the reference's signatures, defaults and shape
conventions (reference interpol/api.py:149-445):

    input : (..., [channel], *inshape)        grid : (..., *outshape, dim)

Batch dimensions broadcast; an input with exactly `dim` dimensions has no
channel axis.  Coordinates are in voxels, component d addresses spatial dim d.

`interpolation`: 0..7 or 'nearest' | 'linear' | 'quadratic' | 'cubic' | 'fourth'
| 'fifth' | 'sixth' | 'seventh' (or a per-dimension list).
`bound`: 'zero' | 'replicate' ('nearest') | 'dct1' ('mirror') | 'dct2' ('reflect')
| 'dst1' ('antimirror') | 'dst2' ('antireflect') | 'dft' ('wrap'), their aliases,
int codes 0..6, or a per-dimension list.
`extrapolate`: False/0 (zero outside the field of view), True/1, or 2 ('hist').

Size limits of this build (the reference has none): one (batch, channel) image -- input of the
gathers, target of the scatters -- must span less than 4 GiB of byte offsets (1024^3 fp32 is just
over, 812^3 fp64 too), spatial strides must stay below 2 GiB, D <= 3, CUDA (HIP) tensors only.
Larger problems raise `ValueError: ... bad or too large extent` from the C-ABI; split them along a
spatial axis (e.g. `interpol.distributed.grid_pull_slabs` for the sample grid) before calling.
(The statement about D and CUDA tensors holds for the HIP kernels: CPU tensors and D > 3 run the
package's PyTorch restatement, `torch_kernels.py`.)

Autograd.  First-order gradients run the fused HIP kernels.  Under `create_graph=True` (double
backward: gradient penalties, Hessian-vector products) the backward is composed from the
differentiable Functions of `autograd.py` instead, as the reference composes its backward from torch
ops (pushpull.py:237-325): the gradient with respect to the grid then materialises `grid_grad`'s
(B, C, *out, D) tensor -- C x D times the memory of the grid, and a second pass.  Third-order
derivatives and beyond through the grid (a backward of that double backward) differentiate on, as
the reference's plain-torch backward does: `GridGrad.backward` under `create_graph=True` lets
autograd differentiate the PyTorch restatement of `grid_grad` (`torch_kernels.py`) -- correct at
any order, at PyTorch speed and memory (the fused kernels carry no graph).
"""
import collections

import torch

from . import backend, ops
from .autograd import (GridPull, GridPush, GridCount, GridGrad, SplineCoeff, SplineCoeffND,
                       AffinePull, AffinePush, AffineCount, Compose, Jacobian, JacDet, Regulariser, RegulariserEnergy,
                       _options, _regulariser_symmetric, regulariser_bound_codes)
from .codes import bound_to_code, order_to_code, pad_codes
from .sepgrid import SeparableGrid, AffineGrid, LazyGrid
from .utils import expanded_shape

__all__ = ['pull', 'push', 'count', 'grid_pull', 'grid_push', 'grid_count', 'grid_grad',
           'spline_coeff', 'spline_coeff_nd', 'compose', 'exp', 'jacobian', 'jacdet', 'regulariser',
           'regulariser_energy', 'regulariser_solve', 'ssd_gauss_newton', 'ssd_gauss_newton_affine', 'mi_gauss_newton_affine',
           'lcc_gauss_newton', 'mi_gauss_newton', 'lcc_gauss_newton_affine']


def _fold(grid, input=None, mode=None):
    """Broadcast and reshape user tensors to the operator layout
    (B, C, *spatial) / (B, *spatial, dim).  Same cases as the reference's
    `_preproc` (interpol/api.py:93-130)."""
    dim = grid.shape[-1]
    if input is None and isinstance(grid, LazyGrid):     # constant lattice: no batch dims, nothing to reshape
        return grid, dict(batch=[], channel=[], dim=dim)
    if input is None:
        spatial = grid.shape[-dim - 1:-1]
        batch = grid.shape[:-dim - 1]
        info = dict(batch=list(batch), channel=[1] if batch else [], dim=dim)
        return grid.reshape([-1, *spatial, dim]), info

    sep = isinstance(grid, LazyGrid)            # constant tensor-product lattice: no batch dims
    grid_spatial = grid.shape[-dim - 1:-1]
    grid_batch = () if sep else grid.shape[:-dim - 1]
    input_spatial = input.shape[-dim:]
    channel = 0 if input.dim() == dim else input.shape[-dim - 1]
    input_batch = input.shape[:-dim - 1]
    if mode == 'push':
        grid_spatial = input_spatial = expanded_shape(grid_spatial, input_spatial)

    batch = expanded_shape(grid_batch, input_batch)
    if not sep:
        grid = grid.expand([*batch, *grid_spatial, dim]).reshape([-1, *grid_spatial, dim])
    input = input.expand([*batch, channel or 1, *input_spatial]).reshape([-1, channel or 1, *input_spatial])
    out_channel = [channel] if channel else ([1] if batch else [])
    return grid, input, dict(batch=list(batch), channel=out_channel, dim=dim)


def _unfold(out, info, mode):
    """Inverse of `_fold` on the result (reference `_postproc`, api.py:133-146)."""
    dim = info['dim']
    if mode == 'grad':
        spatial, feat = out.shape[-dim - 1:-1], [out.shape[-1]]
    else:
        spatial, feat = out.shape[-dim:], []
    return out.reshape([*info['batch'], *info['channel'], *spatial, *feat])


def _learnable(grid, displacement=False):
    """An AffineGrid whose matrix needs a gradient: the operator goes through the Functions that take the matrix as an input
    (autograd.py: AffinePull / AffinePush / AffineCount).  Any other lattice takes the paths it always took.
    `displacement=True` is refused: an AffineGrid holds coordinates (the kernels refuse the two flags together for a
    constant lattice as well), and no path would carry the gradient of the matrix."""
    if not (isinstance(grid, AffineGrid) and grid.requires_grad):
        return False
    if displacement:
        raise ValueError('an AffineGrid holds coordinates: displacement=True cannot be combined with it')
    return True


def _filters(interpolation, dim):
    """Does the prefilter change anything?  Orders 0 and 1 are interpolating already (coeff.py:306-307): the out-of-place
    spline_coeff_nd would only copy the image (0.18 ms for 4 x 2 x 256^3) in front of a gather that does not modify it."""
    codes = [order_to_code(o) for o in (interpolation if isinstance(interpolation, (list, tuple)) else [interpolation])]
    return max(pad_codes(codes, dim)) > 1


def grid_pull(input, grid, interpolation='linear', bound='zero', extrapolate=False, prefilter=False,
              displacement=False):
    """Sample an image at the coordinates of a deformation field.

    input (..., [channel], *inshape), grid (..., *outshape, dim) -> (..., [channel], *outshape).
    Non floating-point inputs are treated as label maps: every label is
    resampled as a soft label and the arg-max is returned (api.py:194-205).

    `displacement=True` (extension, also on grid_push / grid_count / grid_grad): `grid` holds
    voxel displacements and the identity lattice is added inside the kernel -- the fused form of
    `grid_pull(input, add_identity_grid(disp))` (api.py:490-531), same values, one tensor pass less.

    `grid` may be an `interpol.AffineGrid(mat, outshape)` (also on grid_push / grid_count): the lattice
    A o + t is evaluated inside the kernels, and when `mat` requires a gradient it receives one --
    reduced on chip from the per-sample grid gradient, no (*outshape, dim) tensor in either direction.
    """
    if backend.jitfields:
        raise RuntimeError('the jitfields backend is not part of the MI355X build')
    grid, input, info = _fold(grid, input)
    batch, channel = input.shape[:2]
    dim = grid.shape[-1]

    if not input.dtype.is_floating_point:
        codes = [order_to_code(o) for o in (interpolation if isinstance(interpolation, (list, tuple)) else [interpolation])]
        fused = (grid.dtype == torch.float32 and ops.labels_covered(dim, codes, input, grid)
                 and (not prefilter or max(pad_codes(codes, dim)) <= 1)          # order <= 1: the prefilter is the identity
                 and (input.dtype in (torch.bool, torch.uint8, torch.int8, torch.int16, torch.int32)
                      or (input.dtype == torch.int64 and (input.numel() == 0 or int(input.abs().max()) < 2 ** 31))))
        if fused:
            # one pass: arg-max over the labels under each stencil (csrc/labels.hip)
            out = ops.grid_pull_labels(input, grid, [bound_to_code(b) for b in (bound if isinstance(bound, (list, tuple)) else [bound])],
                                       codes, int(extrapolate), displacement).to(input.dtype)
            return _unfold(out, info, 'pull')
        out = input.new_zeros([batch, channel, *grid.shape[1:-1]])
        pmax = grid.new_zeros([batch, channel, *grid.shape[1:-1]])
        for label in input.unique():
            soft = (input == label).to(grid.dtype)
            if prefilter:
                soft = spline_coeff_nd(soft, interpolation=interpolation, bound=bound, dim=dim, inplace=True)
            soft = GridPull.apply(soft, grid, interpolation, bound, extrapolate, displacement)
            out[soft > pmax] = label
            pmax = torch.max(pmax, soft)
    else:
        if prefilter and _filters(interpolation, dim):
            input = spline_coeff_nd(input, interpolation=interpolation, bound=bound, dim=dim)
        if _learnable(grid, displacement):
            out = AffinePull.apply(input, grid.mat, grid.shape[1:-1], interpolation, bound, extrapolate)
        else:
            out = GridPull.apply(input, grid, interpolation, bound, extrapolate, displacement)
    return _unfold(out, info, 'pull')


def grid_push(input, grid, shape=None, interpolation='linear', bound='zero', extrapolate=False,
              prefilter=False, displacement=False):
    """Splat an image along a deformation field (adjoint of `grid_pull`).

    input (..., [channel], *inshape), grid (..., *inshape, dim) -> (..., [channel], *shape);
    `shape` defaults to `inshape`.
    """
    if backend.jitfields:
        raise RuntimeError('the jitfields backend is not part of the MI355X build')
    grid, input, info = _fold(grid, input, mode='push')
    dim = grid.shape[-1]
    if shape is None:
        shape = tuple(input.shape[2:])
    if _learnable(grid, displacement):
        out = AffinePush.apply(input, grid.mat, grid.shape[1:-1], shape, interpolation, bound, extrapolate)
    else:
        out = GridPush.apply(input, grid, shape, interpolation, bound, extrapolate, displacement)
    if prefilter:
        out = spline_coeff_nd(out, interpolation=interpolation, bound=bound, dim=dim, inplace=True)
    return _unfold(out, info, 'push')


def grid_count(grid, shape=None, interpolation='linear', bound='zero', extrapolate=False, displacement=False):
    """Splat ones: grid (..., *inshape, dim) -> (..., [1], *shape)."""
    if backend.jitfields:
        raise RuntimeError('the jitfields backend is not part of the MI355X build')
    grid, info = _fold(grid)
    if _learnable(grid, displacement):
        out = AffineCount.apply(grid.mat, grid.shape[1:-1], shape, interpolation, bound, extrapolate)
    else:
        out = GridCount.apply(grid, shape, interpolation, bound, extrapolate, displacement)
    return _unfold(out, info, 'count')


def grid_grad(input, grid, interpolation='linear', bound='zero', extrapolate=False, prefilter=False,
              displacement=False):
    """Sample the spatial gradient of an image (voxel units):
    input (..., [channel], *inshape), grid (..., *outshape, dim) -> (..., [channel], *outshape, dim).

    An `AffineGrid` whose matrix requires a gradient is expanded to its dense lattice here (`grid.dense()`):
    correct, and slower than the in-kernel lattice -- the gradient of `grid_grad` with respect to the
    coordinates is a Hessian contraction, which has no fused reduction to the matrix."""
    if backend.jitfields:
        raise RuntimeError('the jitfields backend is not part of the MI355X build')
    if _learnable(grid, displacement):
        grid = grid.dense()[0]
    grid, input, info = _fold(grid, input)
    dim = grid.shape[-1]
    if prefilter and _filters(interpolation, dim):
        input = spline_coeff_nd(input, interpolation, bound, dim)
    out = GridGrad.apply(input, grid, interpolation, bound, extrapolate, displacement)
    return _unfold(out, info, 'grad')


def spline_coeff(input, interpolation='linear', bound='dct2', dim=-1, inplace=False):
    """Interpolating B-spline coefficients along ONE dimension.
    Bounds: zero (-> dct1), replicate (-> dct2), dct1, dct2, dft; dst1/dst2 raise
    NotImplementedError (reference interpol/coeff.py:231-254)."""
    if backend.jitfields:
        raise RuntimeError('the jitfields backend is not part of the MI355X build')
    return SplineCoeff.apply(input, bound, interpolation, dim, inplace)


def spline_coeff_nd(input, interpolation='linear', bound='dct2', dim=None, inplace=False):
    """Interpolating B-spline coefficients along the last `dim` dimensions
    (ALL dimensions when `dim` is None)."""
    if backend.jitfields:
        raise RuntimeError('the jitfields backend is not part of the MI355X build')
    return SplineCoeffND.apply(input, bound, interpolation, dim, inplace)


def _fold_fields(*fields):
    """Displacement fields (..., *shape, D) -> (B|1, *shape, D) each, and the broadcast batch shape.  Leading batch dims are
    folded as `_fold` folds those of a grid; a field without batch (or with a batch of ones) stays a batch of 1 that the
    kernels broadcast, so nothing is copied."""
    first = fields[0]
    if not all(torch.is_tensor(f) and f.dtype.is_floating_point for f in fields):
        raise ValueError('displacement fields must be floating point tensors')
    dim = first.shape[-1] if first.dim() else 0
    if dim < 1:
        raise ValueError('a displacement field has shape (..., *spatial, D) with D >= 1, got %s' % list(first.shape))
    for f in fields:
        if f.dtype != first.dtype:
            raise ValueError('displacement fields must share one dtype, got %s and %s' % (first.dtype, f.dtype))
        if f.dim() < dim + 1 or f.shape[-1] != dim:
            raise ValueError('the last dimension of a displacement field must equal its number of spatial dimensions: '
                             'expected (..., *spatial, %d) with %d spatial dims, got %s' % (dim, dim, list(f.shape)))
    batches = [tuple(f.shape[:-dim - 1]) for f in fields]
    batch = batches[0]
    for b in batches[1:]:
        batch = tuple(expanded_shape(batch, b))
    folded = []
    for f, b in zip(fields, batches):
        tail = f.shape[-dim - 1:]
        if all(n == 1 for n in b) and any(n != 1 for n in batch):
            folded.append(f.reshape([1, *tail]))
        else:
            folded.append(f.expand([*batch, *tail]).reshape([-1, *tail]))
    return folded, list(batch), dim


def compose(left, right, interpolation=1, bound='dft', extrapolate=True):
    """Compose two voxel displacement fields defined on one voxel grid (an extension):

        compose(left, right)[o] = right[o] + left(o + right[o])

    left (..., *lshape, D), right (..., *oshape, D) -> (..., *oshape, D); the transformation id + result is
    (id + left) o (id + right).  `left` is interpolated like the image of `grid_pull(..., displacement=True)`: same
    `interpolation`, `bound`, `extrapolate` conventions and per-dim lists; batch dimensions broadcast, fields of one
    floating dtype.  On the GPU, D <= 3, one order 1..3, float32 / float64 run one fused kernel that reads and writes the
    (..., D) layout directly (csrc/compose.hip); everything else is composed from `grid_pull`.  Differentiable in both."""
    if backend.jitfields:
        raise RuntimeError('the jitfields backend is not part of the MI355X build')
    (l, r), batch, dim = _fold_fields(left, right)
    out = Compose.apply(l, r, interpolation, bound, extrapolate)
    return out.reshape([*batch, *out.shape[1:]])


def exp(vel, steps=8, interpolation=1, bound='dft', extrapolate=True, inverse=False):
    """Exponentiate a stationary velocity field (voxels) by scaling and squaring (an extension):
    u_0 = +-vel * 2^-steps, u_{k+1} = compose(u_k, u_k); returns the displacement u_steps, (..., *shape, D) like `vel`.
    `inverse=True` exponentiates -vel.  With a graph every u_k is saved (the usual memory cost of scaling and squaring);
    without one the squarings alternate between two buffers."""
    if backend.jitfields:
        raise RuntimeError('the jitfields backend is not part of the MI355X build')
    steps = int(steps)
    if steps < 0:
        raise ValueError('exp: steps must be >= 0')
    (u,), batch, dim = _fold_fields(vel)
    u = u * ((-1.0 if inverse else 1.0) * 2.0 ** -steps)                   # (an exact power of two)
    if (torch.is_grad_enabled() and u.requires_grad) or torch.is_autocast_enabled():
        for _ in range(steps):
            u = Compose.apply(u, u, interpolation, bound, extrapolate)
    else:
        opt = _options(bound, interpolation, extrapolate)
        other = None
        for _ in range(steps):
            # (the output may alias `right` but not `left`, and a squaring gathers from its own input: two buffers)
            other, u = u, ops.compose(u, u, *opt, out=other)
    return u.reshape([*batch, *u.shape[1:]])


def jacobian(disp, interpolation=1, bound='dft', add_identity=True):
    """Jacobian of the transformation id + disp of a voxel displacement field, at its lattice points (an extension):

        jacobian(disp)[..., o, d, e] = delta_de + d/dx_e u_d (o)

    disp (..., *shape, D) -> (..., *shape, D, D); row `d` is the component, column `e` the direction.  `u_d` is the
    B-spline of order `interpolation` with boundary condition `bound` whose COEFFICIENTS are the values disp[..., d] (no
    prefilter, as `compose` interpolates `left`), and its derivative is taken at the lattice point `o` by the rules of
    `grid_grad` (floor-based first tap): the result is `grid_grad(disp channel-first, identity_grid(shape), interpolation,
    bound, extrapolate=True)` moved to (..., D, D), plus the identity.  So
      - order 1 is the FORWARD difference disp[o + e_e] - disp[o];
      - orders 2 and 3 are the central difference (disp[o + e_e] - disp[o - e_e]) / 2 along `e`, smoothed by
        (1/8, 3/4, 1/8) resp. (1/6, 2/3, 1/6) along the other dims;
      - neighbours beyond a face follow `bound`; lattice points are always in bounds, so there is no `extrapolate`
        argument and no mask.
    `add_identity=False` returns the gradient of disp alone.  `interpolation` and `bound` take per-dim lists; leading batch
    dimensions are free; any floating dtype (16-bit fields compute in float32 and are rounded once).  On the GPU, D <= 3,
    one order listed in `backend.fused_jacobian_orders` and float32 / float64 run one fused kernel that reads and writes
    the (..., D) layout directly (csrc/jacobian.hip); everything else is composed from `grid_grad`.  The one deviation of
    the fused kernel: taps of weight zero are not loaded, so a non-finite value under one does not turn the result into
    NaN as it does in the composed form.  Differentiable (twice) in disp."""
    if backend.jitfields:
        raise RuntimeError('the jitfields backend is not part of the MI355X build')
    (u,), batch, dim = _fold_fields(disp)
    out = Jacobian.apply(u, interpolation, bound, add_identity)
    return out.reshape([*batch, *out.shape[1:]])


def jacdet(disp, interpolation=1, bound='dft'):
    """Determinant of `jacobian(disp)`: disp (..., *shape, D) -> (..., *shape), the local volume change of id + disp
    (<= 0 where it folds); same definition, arguments and routing as `jacobian` (order 1: forward differences).  On the
    GPU the fused kernel expands the determinant in registers: no (..., D, D) field is written.  Differentiable (twice)
    in disp: the gradient is the cofactor matrix times the incoming gradient, pushed back by `grid_pushgrad`."""
    if backend.jitfields:
        raise RuntimeError('the jitfields backend is not part of the MI355X build')
    (u,), batch, dim = _fold_fields(disp)
    out = JacDet.apply(u, interpolation, bound)
    return out.reshape([*batch, *out.shape[1:]])


def _regulariser_args(absolute, membrane, bending, voxel_size, dim, shears=0., div=0.):
    """-> (weights, voxel sizes): three weights where shears = div = 0 (the call of the three-term operator), else five"""
    weights = []
    for name, w in (('absolute', absolute), ('membrane', membrane), ('bending', bending), ('shears', shears), ('div', div)):
        if torch.is_tensor(w):
            raise TypeError('regulariser: `%s` is a plain number (it is not differentiable), got a tensor' % name)
        w = float(w)
        if not 0 <= w < float('inf'):
            raise ValueError('regulariser: `%s` must be a finite non-negative number, got %r' % (name, w))
        weights.append(w)
    vx = [float(h) for h in voxel_size] if isinstance(voxel_size, (list, tuple)) else [float(voxel_size)]
    if len(vx) not in (1, dim):
        raise ValueError('regulariser: `voxel_size` is a number or a list of %d numbers, got %d' % (dim, len(vx)))
    vx = vx * dim if len(vx) == 1 else vx
    if not all(0 < h < float('inf') for h in vx):
        raise ValueError('regulariser: voxel sizes must be positive, got %r' % (vx,))
    if not (weights[3] or weights[4]):
        weights = weights[:3]
    return tuple(weights), tuple(vx)


def regulariser(field, absolute=0., membrane=0., bending=0., voxel_size=1., bound='dft', shears=0., div=0.):
    """The smoothness penalty of a voxel displacement (or velocity) field as a matrix-vector product (an extension; the
    `flow_matvec` / `regulariser` of jitfields and nitorch): field (..., *shape, D) -> L field, (..., *shape, D), with

        (L v)_d = h_d^2 [ absolute v_d + membrane sum_e A_e v_d + bending ( sum_e B_e v_d + sum_{e != f} A_e A_f v_d ) ]
        A_e f [o] = (2 f~[o] - f~[o - e] - f~[o + e]) / h_e^2
        B_e f [o] = (f~[o - 2e] - 4 f~[o - e] + 6 f~[o] - 4 f~[o + e] + f~[o + 2e]) / h_e^4

    The field is in voxels, `voxel_size` h (a number or one per dimension) makes the energy physical.  f~ is the component
    extended along the axis of the stencil by `bound` -- the index and sign rules of every other function (names, aliases, int
    codes, per-dimension lists; one bound per spatial dimension, for every component), applied to every tap of A_e and B_e
    (dst1 keeps the reference's quirk: sign 0 at index 0, the centre tap included).  A_e A_f is the tensor product of the two
    1-D stencils on the extended field: the bending stencil is B_e on the extended field, NOT A_e applied twice (the two differ
    for 'zero' and 'replicate').  In 3-D it has 25 points.

    `absolute`, `membrane`, `bending`: non-negative plain numbers (no tensors, not differentiable); all zero returns zeros
    without a kernel.  Leading batch dimensions are free; any floating dtype (16-bit fields compute in float32 and are rounded
    once).  On the GPU, D <= 3 and float32 / float64 run one fused kernel that reads and writes the (..., D) layout directly
    (csrc/regulariser.hip, `backend.fused_regulariser`); everything else runs the composed form (one index_select per tap).

    L is symmetric positive semi-definite for 'zero', 'dct2', 'dst2', 'dft' and any per-dimension mix of these four.  It is NOT
    symmetric for 'replicate', 'dct1' (three points or more along the dimension) and 'dst1' (two or more): there
    `regulariser_energy` is the quadratic form of a non-symmetric matrix and its gradient is 0.5 (L + L^T) v, not L v.
    Differentiable in `field` any number of times (L is linear: the backward is L^T, the fused kernel again where L is
    symmetric, the transposed composed form else).

    `shears` (mu) and `div` (lambda), non-negative plain numbers: the linear-elastic penalty on the symmetric part of the
    Jacobian of u_c = h_c v_c and on its divergence, E = shears sum eps_ce^2 + div / 2 sum (sum_c d_c u_c)^2, discretised as
    SPM does (compact second differences, and the product of two central differences for the mixed derivatives):

        (L v)_c += h_c^2 [ shears sum_e A_e v_c + (shears + div) A_c v_c ]  -  (shears + div) sum_{e != c} X_ce v_e
        X_ce f [o] = ( f~[o + c + e] - f~[o + c - e] - f~[o - c + e] + f~[o - c - e] ) / 4

    the one term that couples the components.  Its cross taps sit on the in-plane diagonals that bending loads already.
    `bound` also takes 'sliding' (these three functions only), alone or per dimension: in a sliding dimension d, component d
    is extended by 'dst2' along d and every other component by 'dct2' -- the field may slide along the wall but not cross it.
    It applies to every term.  With shears + div > 0, L is symmetric positive semi-definite when every dimension is 'zero',
    'dft' or 'sliding'; it is NOT under 'dct2' or 'dst2' (one bound for every component breaks the cross terms at a
    reflecting wall), nor under 'replicate', 'dct1', 'dst1': it is evaluated all the same, by the same f~ rule, and the
    backward is the transposed composed form there."""
    if backend.jitfields:
        raise RuntimeError('the jitfields backend is not part of the MI355X build')
    (v,), batch, dim = _fold_fields(field)
    weights, vx = _regulariser_args(absolute, membrane, bending, voxel_size, dim, shears, div)
    if not any(weights):
        return torch.zeros_like(field)
    out = Regulariser.apply(v, weights, vx, bound)
    return out.reshape([*batch, *out.shape[1:]])


def regulariser_energy(field, absolute=0., membrane=0., bending=0., voxel_size=1., bound='dft', shears=0., div=0.):
    """0.5 <v, L v> of `regulariser`, one value per batch item: field (..., *shape, D) -> (...); same arguments and routing.
    On the GPU one fused reduction evaluates it without writing L v: every product v_d (L v)_d is formed in the field's
    precision and summed in double in a fixed order, without atomics -- two identical calls give identical bits, and an item
    gives the same bits alone or inside a batch.  For 'replicate', 'dct1' and 'dst1' this is the quadratic form of a
    non-symmetric matrix (see `regulariser`), and so it is for 'dct2' and 'dst2' with `shears` or `div`.  Differentiable in
    `field`: the gradient is 0.5 (L + L^T) v.  `shears`, `div` and bound 'sliding': see `regulariser`."""
    if backend.jitfields:
        raise RuntimeError('the jitfields backend is not part of the MI355X build')
    (v,), batch, dim = _fold_fields(field)
    weights, vx = _regulariser_args(absolute, membrane, bending, voxel_size, dim, shears, div)
    if not any(weights):
        return field.new_zeros(batch)
    return RegulariserEnergy.apply(v, weights, vx, bound).reshape(batch)


SolveInfo = collections.namedtuple('SolveInfo', ['iterations', 'residual'])


def regulariser_solve(gradient, hessian=None, absolute=0., membrane=0., bending=0., voxel_size=1., bound='dft', max_iter=32,
                      tolerance=0., return_info=False, shears=0., div=0., preconditioner='jacobi', smoothing=2):
    """The Gauss-Newton update of a registration step (an extension): x = (H + L)^-1 g by preconditioned conjugate gradients.

    gradient g (..., *shape, D) -> x of the same shape and dtype.  L is exactly the operator of `regulariser`: the same
    `absolute`, `membrane`, `bending`, `shears`, `div` (at least one positive), `voxel_size` and `bound` rules -- but only the
    bounds for which L is symmetric: 'zero', 'dft', 'sliding', without `shears` and `div` also 'dct2' and 'dst2', and
    per-dimension mixes of them (anything else raises ValueError: conjugate gradients need a symmetric matrix).  `hessian` is None (H = 0) or (..., *shape, K) of the dtype of `gradient`:
    K = D is a diagonal Hessian, K = D (D + 1) / 2 a symmetric one, the diagonal first and then the upper triangle row by row
    ((0,1), (0,2), (1,2) in 3-D); for D = 1 both are K = 1.  H must be positive semi-definite at every voxel: this is NOT
    checked, and an indefinite H may give non-finite values (never an access outside the buffers).  Batch dimensions broadcast;
    a Hessian without a batch serves every item and is not copied.

    The algorithm, for each batch item on its own (inner products are sums of double products; alpha and beta are doubles,
    rounded to the field's precision once where they multiply a field):

        c_d = h_d^2 [ absolute + membrane sum_e 2 / h_e^2 + bending ( sum_e 6 / h_e^4 + sum_{e != f} 4 / (h_e^2 h_f^2) )
                      + shears sum_e 2 / h_e^2 + (shears + div) 2 / h_d^2 ]
        M_o = H_o + diag(c)                                  (the interior diagonal of L; inverted per voxel in closed form)
        x = 0;  r = g;  z = M^-1 r;  p = z;  rho = <r,z>;  gamma = <g,g>;  done = (gamma == 0)
        for k = 1 .. max_iter, items not done:
            q = (H + L) p;   pi = <p,q>;   if pi <= 0 or rho <= 0: done, skip
            alpha = rho / pi;  x += alpha p;  r -= alpha q;  z = M^-1 r;  rho' = <r,z>;  sigma = <r,r>;  iterations += 1
            if sigma <= tolerance^2 gamma: done
            beta = rho' / rho;  rho = rho';  p = z + beta p

    `max_iter`: an int >= 0 (0 returns zeros); `tolerance`: a float >= 0, the relative residual sqrt(sigma / gamma) at which an
    item stops.  `return_info=True` returns (x, info): `info.iterations` (int64, the batch shape) counts the iterations that
    changed x, `info.residual` (float64, the batch shape) is sqrt(sigma / gamma), 0 where gamma = 0 or no iteration ran.  Both are
    device tensors: nothing in the call synchronises with the host, so it can be captured in a graph.

    `preconditioner='multigrid'` replaces z = M^-1 r by z = V(r), one multigrid V-cycle, in the initialisation and in the loop;
    everything else above is unchanged.  The iteration count of 'jacobi' grows with the lattice, that of 'multigrid' hardly does
    (bending, 64 x 64: more than 400 against 16).  The cycle, with omega = 1/2 and nu = `smoothing` (an int >= 1):

        levels: level 0 is the lattice; dimension d is halved iff n_d is even and n_d / 2 >= 4, else it keeps its size; the last
            level is the one on which nothing can be halved.  s_d = 2 where halved, else 1; h_{l+1,d} = s_d h_{l,d};
            kappa_{l+1} = kappa_l prod_d s_d (kappa_0 = 1)
        A_l = H_l + L(kappa_l weights, h_l, bound);   M_l = H_l + diag(c(kappa_l weights, h_l))
        P_l (coarse to fine, component c): along each halved dimension fine i = 3/4 e[i >> 1] + 1/4 e[(i >> 1) -+ 1] (minus for
            even i), a coarse index out of range extended by the bound of the dimension for that component; times s_c
        H_{l+1}[o] = S (sum over the children of o of H_l) S,  S = diag(s)
        V(l, r): x = 0;  nu sweeps x <- x + omega M_l^-1 (r - A_l x)   (8 on the last level, which returns x)
                 d = r - A_l x;  x <- x + P_l V(l + 1, P_l^T d);  nu more sweeps

    On the GPU, D <= 3 and float32 / float64 run fused kernels for it as well (csrc/regulariser_multigrid.hip,
    `backend.fused_regulariser_multigrid`).  Any other `preconditioner`, or a `smoothing` that is not an int >= 1, raises ValueError.

    On the GPU, D <= 3 and float32 / float64 run the fused kernels (csrc/regulariser_solve.hip, `backend.fused_regulariser_solve`:
    every iteration enqueued from one call, the scalars on the device); everything else runs the composed form, the same
    algorithm around `regulariser` (16-bit fields compute in float32 and are rounded once).  NOT differentiable: with grad mode
    on and an input that requires grad it raises RuntimeError (call it under torch.no_grad(), or detach)."""
    if backend.jitfields:
        raise RuntimeError('the jitfields backend is not part of the MI355X build')
    tensors = [gradient] if hessian is None else [gradient, hessian]
    if not all(torch.is_tensor(t) and t.dtype.is_floating_point for t in tensors):
        raise ValueError('regulariser_solve: `gradient` and `hessian` must be floating point tensors')
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        raise RuntimeError('regulariser_solve is not differentiable: call it under torch.no_grad() or detach its inputs')
    (g,), gbatch, dim = _fold_fields(gradient)
    weights, vx = _regulariser_args(absolute, membrane, bending, voxel_size, dim, shears, div)
    if not any(weights):
        raise ValueError('regulariser_solve: at least one of `absolute`, `membrane`, `bending`, `shears`, `div` must be positive '
                         '(without L the system is a pointwise solve)')
    codes = regulariser_bound_codes(bound, dim)
    if not _regulariser_symmetric(codes, weights):
        raise ValueError("regulariser_solve: conjugate gradients need a symmetric L: every bound must be one of 'zero', 'dft', "
                         "'sliding', or without `shears` and `div` 'dct2', 'dst2', got %r" % (bound,))
    if isinstance(max_iter, bool) or not isinstance(max_iter, int) or max_iter < 0:
        raise ValueError('regulariser_solve: `max_iter` is an int >= 0, got %r' % (max_iter,))
    if torch.is_tensor(tolerance) or not float(tolerance) >= 0 or float(tolerance) == float('inf'):
        raise ValueError('regulariser_solve: `tolerance` is a finite float >= 0, got %r' % (tolerance,))
    if preconditioner not in ('jacobi', 'multigrid'):
        raise ValueError("regulariser_solve: `preconditioner` is 'jacobi' or 'multigrid', got %r" % (preconditioner,))
    if isinstance(smoothing, bool) or not isinstance(smoothing, int) or smoothing < 1:
        raise ValueError('regulariser_solve: `smoothing` is an int >= 1, got %r' % (smoothing,))
    batch, h = gbatch, None
    if hessian is not None:
        if hessian.dtype != gradient.dtype or hessian.device != gradient.device:
            raise ValueError('regulariser_solve: `hessian` must have the dtype and device of `gradient`, got %s on %s and %s on %s'
                             % (hessian.dtype, hessian.device, gradient.dtype, gradient.device))
        K = hessian.shape[-1] if hessian.dim() else 0
        if K not in (dim, dim * (dim + 1) // 2):
            raise ValueError('regulariser_solve: the last dimension of `hessian` is %d (diagonal) or %d (symmetric), got %d'
                             % (dim, dim * (dim + 1) // 2, K))
        if hessian.dim() < dim + 1 or tuple(hessian.shape[-dim - 1:-1]) != tuple(gradient.shape[-dim - 1:-1]):
            raise ValueError('regulariser_solve: `hessian` must have the spatial shape of `gradient`, got %s and %s'
                             % (list(hessian.shape), list(gradient.shape)))
        hbatch = tuple(hessian.shape[:-dim - 1])
        batch = list(expanded_shape(tuple(gbatch), hbatch))
        tail = hessian.shape[-dim - 1:]
        if all(n == 1 for n in hbatch) and any(n != 1 for n in batch):
            h = hessian.reshape([1, *tail])                             # (one Hessian for every item: not copied)
        else:
            h = hessian.expand([*batch, *tail]).reshape([-1, *tail])
        if list(batch) != list(gbatch):
            g = gradient.expand([*batch, *gradient.shape[-dim - 1:]]).reshape([-1, *gradient.shape[-dim - 1:]])
    with torch.no_grad():
        if preconditioner == 'multigrid':
            x, iterations, residual = ops.regulariser_multigrid(g, h, weights, vx, codes, max_iter, float(tolerance), smoothing)
        else:
            x, iterations, residual = ops.regulariser_solve(g, h, weights, vx, codes, max_iter, float(tolerance))
    x = x.reshape([*batch, *x.shape[1:]])
    if return_info:
        return x, SolveInfo(iterations.reshape(batch), residual.reshape(batch))
    return x


def _fold_batch(t, nbatch, batch):
    """(*own batch, *tail) -> (B|1, *tail): an operand without a batch (or with a batch of ones) stays a batch of 1 that the
    kernels broadcast, so nothing is copied; `nbatch`: how many leading dims are batch dims."""
    own, tail = tuple(t.shape[:nbatch]), list(t.shape[nbatch:])
    if all(n == 1 for n in own) and any(n != 1 for n in batch):
        return t.reshape([1, *tail])
    return t.expand([*batch, *tail]).reshape([-1, *tail])


def _data_term_operands(name, moving, fixed, disp, weight, hessian):
    """The checks that `ssd_gauss_newton` and `lcc_gauss_newton` share -> (dim, nb, batch): the number of spatial dims, the number
    of batch dims of (moving, fixed, disp[, weight]) and the broadcast batch."""
    if backend.jitfields:
        raise RuntimeError('the jitfields backend is not part of the MI355X build')
    names = ['moving', 'fixed', 'disp'] + ([] if weight is None else ['weight'])
    tensors = [moving, fixed, disp] + ([] if weight is None else [weight])
    if not all(torch.is_tensor(t) and t.dtype.is_floating_point for t in tensors):
        raise ValueError(name + ': `moving`, `fixed`, `disp` and `weight` must be floating point tensors')
    for n, t in zip(names, tensors):
        if t.dtype != disp.dtype or t.device != disp.device:
            raise ValueError(name + ': `%s` must have the dtype and device of `disp`, got %s on %s and %s on %s'
                             % (n, t.dtype, t.device, disp.dtype, disp.device))
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        raise RuntimeError(name + ' is not differentiable: call it under torch.no_grad() or detach its inputs')
    if hessian not in (None, 'diagonal', 'full'):
        raise ValueError(name + ": `hessian` is 'full', 'diagonal' or None, got %r" % (hessian,))
    dim = disp.shape[-1] if disp.dim() else 0
    if dim < 1 or disp.dim() < dim + 1 or fixed.dim() < dim + 1 or moving.dim() < dim + 1:
        raise ValueError(name + ': the last dimension of `disp` must equal the number of spatial dimensions: `disp` '
                         '(..., *shape, D), `moving` (..., C, *inshape), `fixed` (..., C, *shape), got %s, %s and %s'
                         % (list(disp.shape), list(moving.shape), list(fixed.shape)))
    shape = tuple(disp.shape[-dim - 1:-1])
    if tuple(fixed.shape[-dim:]) != shape:
        raise ValueError(name + ': `fixed` and `disp` must share the spatial shape, got %s and %s'
                         % (list(fixed.shape), list(disp.shape)))
    if weight is not None and (weight.dim() < dim or tuple(weight.shape[-dim:]) != shape):
        raise ValueError(name + ': `weight` must have the spatial shape of `fixed`, got %s and %s'
                         % (list(weight.shape), list(fixed.shape)))
    if moving.shape[-dim - 1] != fixed.shape[-dim - 1]:
        raise ValueError(name + ': `moving` and `fixed` must have the same number of channels, got %d and %d'
                         % (moving.shape[-dim - 1], fixed.shape[-dim - 1]))
    nb = [moving.dim() - dim - 1, fixed.dim() - dim - 1, disp.dim() - dim - 1] + ([] if weight is None else [weight.dim() - dim])
    batch = ()
    for t, n in zip(tensors, nb):
        batch = tuple(expanded_shape(batch, tuple(t.shape[:n])))
    return dim, nb, batch


def ssd_gauss_newton(moving, fixed, disp, weight=None, interpolation=1, bound='dct2', extrapolate=True, prefilter=False,
                     hessian='full'):
    """The sum-of-squares data term of a Gauss-Newton registration step (an extension): loss, gradient and Hessian in one pass.

    moving (..., C, *inshape), fixed (..., C, *shape), disp (..., *shape, D) voxel displacements on the lattice of `fixed` (the two
    lattices may differ in shape), weight None or (..., *shape), broadcast over the channels (its sign is not checked)
    -> (loss (...), gradient (..., *shape, D), hessian (..., *shape, K) | None).  With

        w = grid_pull(moving, disp, displacement=True, ...),  G = grid_grad(moving, disp, displacement=True, ...),  r = w - fixed

        loss            = 1/2 sum_o sum_c weight(o) r_c(o)^2          one value per batch item, no normalisation
        gradient[o, d]  = weight(o) sum_c r_c(o) G_cd(o)              = d loss / d disp exactly
        hessian[o, k]   = weight(o) sum_c G_cd(o) G_ce(o)

    Out-of-view samples under `extrapolate=False` have w = 0 and G = 0 as in grid_pull / grid_grad: r = -fixed and a zero
    gradient and Hessian.  `hessian='full'`: K = D (D + 1) / 2, the diagonal first and then the upper triangle row by row --
    what `regulariser_solve(hessian=...)` takes; 'diagonal': K = D; None: no Hessian is computed and the third item is None.
    `interpolation`, `bound` (per-dimension lists and every alias), `extrapolate` as for grid_pull; `prefilter=True` runs
    `spline_coeff_nd` on `moving` first (orders above 1).  Batch dimensions broadcast; an operand without a batch is not
    copied.  All tensors share one floating dtype and one device.

    On the GPU, D <= 3, float32 / float64 and one order out of `backend.fused_ssd_orders` (without a Hessian: out of
    `backend.fused_ssd_orders_without_hessian` as well; both measured, profiles/ssd.txt) run one fused kernel (csrc/ssd.hip:
    one stencil per sample for every channel, w and G never stored; the loss is summed in double in a fixed order, without
    atomics -- two calls give identical bits, and an item gives the same bits alone or inside a batch); everything else runs the
    composed form above (16-bit tensors compute in float32 and are rounded once).  NOT differentiable: with grad mode on and
    an input that requires grad it raises RuntimeError (call it under torch.no_grad(), or detach)."""
    dim, nb, batch = _data_term_operands('ssd_gauss_newton', moving, fixed, disp, weight, hessian)
    with torch.no_grad():
        if prefilter and _filters(interpolation, dim):
            moving = spline_coeff_nd(moving, interpolation=interpolation, bound=bound, dim=dim)
        m, f, u = (_fold_batch(t, n, batch) for t, n in zip((moving, fixed, disp), nb))
        w = None if weight is None else _fold_batch(weight, nb[3], batch)
        loss, gradient, hess = ops.ssd_gauss_newton(m, f, u, w, *_options(bound, interpolation, extrapolate), hessian)
    loss = loss.reshape(batch)
    gradient = gradient.reshape([*batch, *gradient.shape[1:]])
    if hess is not None:
        hess = hess.reshape([*batch, *hess.shape[1:]])
    return loss, gradient, hess


def lcc_gauss_newton(moving, fixed, disp, weight=None, window=9, interpolation=1, bound='dct2', extrapolate=True, prefilter=False,
                     hessian='full', eps=1e-5):
    """The local (windowed) normalised cross-correlation data term of a Gauss-Newton registration step (an extension): loss,
    gradient and the positive part of the Hessian.  ANTs' "CC", VoxelMorph's "NCC": invariant to a local affine change of intensity.

    moving (..., C, *inshape), fixed (..., C, *shape), disp (..., *shape, D) voxel displacements on the lattice of `fixed`, weight
    None or (..., *shape), broadcast over the channels -> (loss (...), gradient (..., *shape, D), hessian (..., *shape, K) | None).
    `window`: an odd integer >= 1, or one per spatial dimension; r_d = (window_d - 1) / 2.  `eps` > 0.  With

        I = grid_pull(moving, disp, displacement=True, ...),  G = grid_grad(moving, disp, displacement=True, ...),  J = fixed

    and for every channel on its own

        W(o)   = {p in the lattice: |p_d - o_d| <= r_d for all d}   clipped at the edges, not wrapped;  n(o) = |W(o)|
        S_X(o) = sum_{p in W(o)} X(p)   for X in I, J, I^2, J^2, IJ                           ("box")
        cross  = S_IJ - S_I S_J / n,  vI = max(S_II - S_I^2 / n, 0),  vJ = max(S_JJ - S_J^2 / n, 0),  den = vI vJ + eps
        cc     = cross^2 / den                                                               0 <= cc <= 1
        a = weight 2 cross / den,  c = weight 2 cross^2 vJ / den^2,  f = (a S_J - c S_I) / n;   A, C, F = box(a), box(c), box(f)
        dI(p)  = -J(p) A(p) + I(p) C(p) + F(p)

        loss            = - sum_o weight(o) sum_c cc_c(o)             one value per batch item, no normalisation
        gradient[p, d]  = sum_c dI_c(p) G_cd(p)                       = d loss / d disp exactly (where no max(., 0) is active)
        hessian[p, k]   = sum_c C_c(p) G_cd(p) G_ce(p)                positive semi-definite for weight >= 0

    `hessian` keeps the positive diagonal part of d^2 loss / d I^2 (the other second-order terms are indefinite): what
    `regulariser_solve(hessian=...)` takes.  'full': K = D (D + 1) / 2, the diagonal first and then the upper triangle row by row;
    'diagonal': K = D; None: the third item is None.  Out-of-view samples under `extrapolate=False` have I = 0 and G = 0 and enter
    the window sums as zeros.  `interpolation`, `bound`, `extrapolate`, `prefilter`, the batch broadcasting and the dtype and
    device rules as for `ssd_gauss_newton`.

    Precision: the five window sums and everything down to a, c, f -- the loss included -- are formed in float64 from I and J of
    the tensors' dtype (S_II - S_I^2 / n cancels: in float32 the gradient of an image whose mean is ten standard deviations is wrong);
    a, c, f stay float64; A, C, F are summed in float64; dI and the outputs are in the dtype.

    On the GPU, D <= 3, float32 / float64, odd windows up to 9 and one order out of `backend.fused_lcc_orders` (measured,
    profiles/lcc.txt) run the fused kernels (csrc/lcc.hip: a pull, and two marches of a workgroup-owned tile with the window sums
    in LDS; no atomics, every sum in a fixed order -- two calls give identical bits, and an item gives the same bits alone or
    inside a batch); everything else runs the composed form (`torch_kernels.lcc_gauss_newton_composed`; 16-bit tensors compute in
    float32 and are rounded once).  NOT differentiable: with grad mode on and an input that requires grad it raises RuntimeError."""
    dim, nb, batch = _data_term_operands('lcc_gauss_newton', moving, fixed, disp, weight, hessian)
    if isinstance(window, (list, tuple)):
        window = list(window)
        if len(window) != dim:
            raise ValueError('lcc_gauss_newton: `window` is one odd integer or one per spatial dimension (%d), got %r' % (dim, window))
    else:
        window = [window] * dim
    if not all(isinstance(w, int) and not isinstance(w, bool) and w >= 1 and w % 2 == 1 for w in window):
        raise ValueError('lcc_gauss_newton: `window` must be odd integers >= 1, got %r' % (window,))
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not (0 < float(eps) < float('inf')):
        raise ValueError('lcc_gauss_newton: `eps` is a finite float > 0, got %r' % (eps,))
    with torch.no_grad():
        if prefilter and _filters(interpolation, dim):
            moving = spline_coeff_nd(moving, interpolation=interpolation, bound=bound, dim=dim)
        m, f, u = (_fold_batch(t, n, batch) for t, n in zip((moving, fixed, disp), nb))
        w = None if weight is None else _fold_batch(weight, nb[3], batch)
        loss, gradient, hess = ops.lcc_gauss_newton(m, f, u, w, *_options(bound, interpolation, extrapolate), hessian, window, float(eps))
    loss = loss.reshape(batch)
    gradient = gradient.reshape([*batch, *gradient.shape[1:]])
    if hess is not None:
        hess = hess.reshape([*batch, *hess.shape[1:]])
    return loss, gradient, hess


def _affine_term_operands(name, moving, fixed, mat, weight):
    """The checks that `ssd_gauss_newton_affine` and `lcc_gauss_newton_affine` share -> (dim, mat[..., :D, :], the number of batch
    dimensions of each operand, the broadcast batch shape)."""
    if backend.jitfields:
        raise RuntimeError('the jitfields backend is not part of the MI355X build')
    names = ['moving', 'fixed', 'mat'] + ([] if weight is None else ['weight'])
    tensors = [moving, fixed, mat] + ([] if weight is None else [weight])
    if not all(torch.is_tensor(t) and t.dtype.is_floating_point for t in tensors):
        raise ValueError(name + ': `moving`, `fixed`, `mat` and `weight` must be floating point tensors')
    for n, t in zip(names, tensors):
        if t.dtype != mat.dtype or t.device != mat.device:
            raise ValueError(name + ': `%s` must have the dtype and device of `mat`, got %s on %s and %s on %s'
                             % (n, t.dtype, t.device, mat.dtype, mat.device))
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        raise RuntimeError(name + ' is not differentiable: call it under torch.no_grad() or detach its inputs')
    dim = mat.shape[-1] - 1 if mat.dim() >= 2 else 0
    if dim < 1 or mat.shape[-2] not in (dim, dim + 1) or fixed.dim() < dim + 1 or moving.dim() < dim + 1:
        raise ValueError(name + ': `mat` (..., D or D+1, D+1) sets the number of spatial dimensions: `moving` '
                         '(..., C, *inshape), `fixed` (..., C, *shape), got %s, %s and %s'
                         % (list(mat.shape), list(moving.shape), list(fixed.shape)))
    shape = tuple(fixed.shape[-dim:])
    if weight is not None and (weight.dim() < dim or tuple(weight.shape[-dim:]) != shape):
        raise ValueError(name + ': `weight` must have the spatial shape of `fixed`, got %s and %s'
                         % (list(weight.shape), list(fixed.shape)))
    if moving.shape[-dim - 1] != fixed.shape[-dim - 1]:
        raise ValueError(name + ': `moving` and `fixed` must have the same number of channels, got %d and %d'
                         % (moving.shape[-dim - 1], fixed.shape[-dim - 1]))
    mat = mat[..., :dim, :]
    nb = [moving.dim() - dim - 1, fixed.dim() - dim - 1, mat.dim() - 2] + ([] if weight is None else [weight.dim() - dim])
    batch = ()
    for t, n in zip(tensors, nb):
        batch = tuple(expanded_shape(batch, tuple(t.shape[:n])))
    return dim, mat, nb, batch


def ssd_gauss_newton_affine(moving, fixed, mat, weight=None, interpolation=1, bound='dct2', extrapolate=True, prefilter=False,
                            hessian=True):
    """The sum-of-squares data term of a Gauss-Newton step on an AFFINE lattice (an extension): loss, gradient of the matrix
    entries and their Gauss-Newton Hessian in one pass over the samples.

    moving (..., C, *inshape), fixed (..., C, *shape), mat (..., D or D+1, D+1) with D = mat.shape[-1] - 1 (a last row, if present,
    is ignored, as in `AffineGrid`; ONE MATRIX PER BATCH ITEM is allowed), weight None or (..., *shape), broadcast over the channels
    -> (loss (...), gradient (..., D, D+1), hessian (..., P, P) | None), P = D (D+1).  Sample o of item b sits at x = A_b o + t_b,
    formed exactly as `AffineGrid` forms it (in the tensors' dtype, fused multiply-adds).  With o~ = (o_0 .. o_{D-1}, 1) and

        w = grid_pull(moving, x, ...),  G = grid_grad(moving, x, ...),  r = w - fixed

        loss                                = 1/2 sum_o weight sum_c r_c^2               one value per batch item, no normalisation
        gradient[d, e]                      = sum_o weight sum_c r_c G_cd o~_e           = d loss / d mat[:D] exactly
        hessian[d (D+1) + e, d' (D+1) + e'] = sum_o weight sum_c G_cd G_cd' o~_e o~_e'   the index order of gradient.reshape(P)

    The Hessian is the full matrix, both triangles written from the same sum: exactly symmetric.  `hessian=False` computes none and
    the third item is None.  Out-of-view samples under `extrapolate=False` have w = 0 and G = 0 as in `ssd_gauss_newton`.
    `interpolation`, `bound` (per-dimension lists and every alias), `extrapolate` as for grid_pull; `prefilter=True` runs
    `spline_coeff_nd` on `moving` first (orders above 1).  Batch dimensions broadcast; an operand without a batch is not copied.
    All tensors share one floating dtype and one device.  A plain Gauss-Newton loop:

        mat = torch.eye(D + 1, dtype=moving.dtype, device=moving.device)[:D]
        for _ in range(10):
            loss, g, H = ssd_gauss_newton_affine(moving, fixed, mat, interpolation=3)
            step = torch.linalg.solve(H.double(), g.reshape(-1).double())
            mat = mat - step.reshape(D, D + 1).to(mat.dtype)

    On the GPU, D <= 3, float32 / float64 and one order out of `backend.fused_ssd_affine_orders` (measured,
    profiles/ssd_affine.txt) run one fused kernel (csrc/ssd_affine.hip: nothing of size N but the images is touched; the 1 + P
    + 60 sums of a 3-D item are kept in double and reduced in a fixed order, without atomics -- two calls give identical bits, and
    an item gives the same bits alone or inside a batch); everything else runs the composed form
    (`torch_kernels.ssd_gauss_newton_affine_composed`: a dense lattice, `ssd_gauss_newton` and two float64 contractions; 16-bit
    tensors compute in float32 and are rounded once).  NOT differentiable: with grad mode on and an input that requires grad it
    raises RuntimeError (call it under torch.no_grad(), or detach); the chain rule from the matrix entries to another
    parametrisation is the caller's."""
    dim, mat, nb, batch = _affine_term_operands('ssd_gauss_newton_affine', moving, fixed, mat, weight)
    with torch.no_grad():
        if prefilter and _filters(interpolation, dim):
            moving = spline_coeff_nd(moving, interpolation=interpolation, bound=bound, dim=dim)
        m, f, a = (_fold_batch(t, n, batch) for t, n in zip((moving, fixed, mat), nb))
        w = None if weight is None else _fold_batch(weight, nb[3], batch)
        loss, gradient, hess = ops.ssd_gauss_newton_affine(m, f, a, w, *_options(bound, interpolation, extrapolate), bool(hessian))
    loss = loss.reshape(batch)
    gradient = gradient.reshape([*batch, dim, dim + 1])
    if hess is not None:
        hess = hess.reshape([*batch, *hess.shape[1:]])
    return loss, gradient, hess


def lcc_gauss_newton_affine(moving, fixed, mat, weight=None, window=9, interpolation=1, bound='dct2', extrapolate=True,
                            prefilter=False, hessian=True, eps=1e-5):
    """The local (windowed) normalised cross-correlation data term of a Gauss-Newton step on an AFFINE lattice (an extension): the
    loss of `lcc_gauss_newton`, its gradient with respect to the matrix entries and the positive part of their Hessian.  Invariant
    to a local affine change of intensity: the data term of the affine stage between scans of one modality from different scanners.

    moving (..., C, *inshape), fixed (..., C, *shape), mat (..., D or D+1, D+1) with D = mat.shape[-1] - 1 (a last row, if present,
    is ignored, as in `AffineGrid`; ONE MATRIX PER BATCH ITEM is allowed), weight None or (..., *shape), broadcast over the channels
    -> (loss (...), gradient (..., D, D+1), hessian (..., P, P) | None), P = D (D+1).  `window`: an odd integer >= 1, or one per
    spatial dimension; `eps` > 0.  Sample o of item b sits at x = A_b o + t_b, formed exactly as `AffineGrid` forms it.  With

        I = grid_pull(moving, x, ...),  G = grid_grad(moving, x, ...),  J = fixed,  o~ = (o_0 .. o_{D-1}, 1)

    and the window sums, cc, a, c, f, A, C, F and dI exactly as `lcc_gauss_newton` defines them at those coordinates:

        loss                                = - sum_o weight sum_c cc_c(o)               the dense term's loss
        gradient[d, e]                      = sum_o sum_c dI_c(o) G_cd(o) o~_e           = d loss / d mat[:D] (where no max(., 0) is active)
        hessian[d (D+1) + e, d' (D+1) + e'] = sum_o sum_c C_c(o) G_cd(o) G_cd'(o) o~_e o~_e'   the index order of gradient.reshape(P)

    The Hessian is the positive part that the dense term keeps, contracted: positive semi-definite for weight >= 0 and conservative
    (a plain Gauss-Newton iteration converges linearly).  It is the full matrix, both triangles written from the same sum: exactly
    symmetric.  `hessian=False` computes none and the third item is None.  Out-of-view samples under `extrapolate=False` have I = 0
    and G = 0 and enter the window sums as zeros.  `interpolation`, `bound`, `extrapolate`, `prefilter`, the batch broadcasting and
    the dtype and device rules as for `ssd_gauss_newton_affine`.  A plain Gauss-Newton loop:

        mat = torch.eye(D + 1, dtype=moving.dtype, device=moving.device)[:D]
        for _ in range(20):
            loss, g, H = lcc_gauss_newton_affine(moving, fixed, mat, interpolation=3)
            step = torch.linalg.solve(H.double(), g.reshape(-1).double())
            mat = mat - step.reshape(D, D + 1).to(mat.dtype)

    Precision: I, the window sums, a, c, f, the loss and A, C, F as for `lcc_gauss_newton`; dI and C are rounded to the dtype once
    per sample; G and the per-sample products are formed in the dtype, converted to double once and summed in double.

    On the GPU, D <= 3, float32 / float64, odd windows up to 9 and one order out of `backend.fused_lcc_affine_orders` (measured,
    profiles/lcc_affine.txt) run the fused kernels (csrc/lcc_affine.hip: the pull and the statistics of `lcc_gauss_newton`, a march
    that stores dI and C per sample, and the sums of `ssd_gauss_newton_affine` with one stencil per sample; no lattice, no gradient
    or Hessian field; no atomics, every sum in a fixed order -- two calls give identical bits, and an item gives the same bits alone
    or inside a batch); everything else runs the composed form (`torch_kernels.lcc_gauss_newton_affine_composed`: a dense lattice,
    `lcc_gauss_newton` and two float64 contractions; 16-bit tensors compute in float32 and are rounded once).  NOT differentiable:
    with grad mode on and an input that requires grad it raises RuntimeError (call it under torch.no_grad(), or detach)."""
    name = 'lcc_gauss_newton_affine'
    dim, mat, nb, batch = _affine_term_operands(name, moving, fixed, mat, weight)
    if isinstance(window, (list, tuple)):
        window = list(window)
        if len(window) != dim:
            raise ValueError(name + ': `window` is one odd integer or one per spatial dimension (%d), got %r' % (dim, window))
    else:
        window = [window] * dim
    if not all(isinstance(w, int) and not isinstance(w, bool) and w >= 1 and w % 2 == 1 for w in window):
        raise ValueError(name + ': `window` must be odd integers >= 1, got %r' % (window,))
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not (0 < float(eps) < float('inf')):
        raise ValueError(name + ': `eps` is a finite float > 0, got %r' % (eps,))
    with torch.no_grad():
        if prefilter and _filters(interpolation, dim):
            moving = spline_coeff_nd(moving, interpolation=interpolation, bound=bound, dim=dim)
        m, f, a = (_fold_batch(t, n, batch) for t, n in zip((moving, fixed, mat), nb))
        w = None if weight is None else _fold_batch(weight, nb[3], batch)
        loss, gradient, hess = ops.lcc_gauss_newton_affine(m, f, a, w, *_options(bound, interpolation, extrapolate), bool(hessian),
                                                           window, float(eps))
    loss = loss.reshape(batch)
    gradient = gradient.reshape([*batch, dim, dim + 1])
    if hess is not None:
        hess = hess.reshape([*batch, *hess.shape[1:]])
    return loss, gradient, hess


def _mi_options(name, bins, moving_range, fixed_range):
    """The checks of `bins` and the two ranges that `mi_gauss_newton_affine` and `mi_gauss_newton` share."""
    if isinstance(bins, bool) or not isinstance(bins, int) or bins < 8:
        raise ValueError(name + ': `bins` is an integer >= 8, got %r' % (bins,))
    for n, r in (('moving_range', moving_range), ('fixed_range', fixed_range)):
        if r is not None and not (isinstance(r, (tuple, list)) and len(r) == 2
                                  and all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in r)):
            raise ValueError(name + ': `%s` is None or a pair of floats (lo, hi), got %r' % (n, r))


def mi_gauss_newton_affine(moving, fixed, mat, weight=None, bins=32, moving_range=None, fixed_range=None, interpolation=1,
                           bound='dct2', extrapolate=True, prefilter=False, hessian=True, return_histogram=False):
    """The mutual-information data term of a step on an AFFINE lattice (an extension): minus the mutual information of the joint
    Parzen histogram of moving(A o + t) and fixed, its gradient with respect to the matrix entries and a majoriser of their
    Hessian.  Invariant to the intensity scale of either image: the data term of a multi-modal affine alignment.

    moving (..., 1, *inshape), fixed (..., 1, *shape) -- ONE channel --, mat (..., D or D+1, D+1) with D = mat.shape[-1] - 1 (a last
    row, if present, is ignored; one matrix per batch item is allowed), weight None or (..., *shape), weight >= 0 (not checked)
    -> (loss (...), gradient (..., D, D+1), hessian (..., P, P) | None), P = D (D+1); with `return_histogram=True` also the joint
    histogram (..., bins, bins) as a fourth item.  `bins` = B: an integer >= 8.  The lattice and the interpolated image are those
    of `ssd_gauss_newton_affine`:

        x(o) = A o + t,   I = grid_pull(moving, x, ...),   G = grid_grad(moving, x, ...),   J = fixed,   o~ = (o_0 .. o_{D-1}, 1)
        m(o) the in-view mask of grid_pull (1 under extrapolate=True),   omega = weight m,   W = sum_o omega

    Ranges: `moving_range` / `fixed_range` are pairs of floats (lo, hi); None = `torch.aminmax` of the tensor per batch item, kept
    on the device (no host synchronisation).  A degenerate range (hi <= lo) gives t = 0.

        t_m = clamp((I - m_lo) / (m_hi - m_lo), 0, 1),   t_f = clamp((J - f_lo) / (f_hi - f_lo), 0, 1)
        k(o) = floor(t_f (B - 1) + 1/2)  in 0 .. B-1                                  fixed side: a window of order 0
        u(o) = 1.5 + t_m (B - 4),  taps j = floor(u) - 1 .. floor(u) + 2  in 0 .. B-1   moving side: the cubic B-spline beta3,
                                                                                      whose four weights beta3(u - j) sum to 1
        P[j, k] = sum_o omega beta3(u - j) [k = k(o)] / W          out-of-view samples are excluded, not counted as zeros
        p_m = sum_k P,   p_f = sum_j P,   T[j, k] = log(P / (p_m p_f)) where P > 0, else 0
        loss = - sum_jk P T                                         one value per batch item; W <= 0: every output is zero

        s = (B - 4) / (m_hi - m_lo), 0 for a sample whose t_m was clamped
        dI(o) = -(omega / W) s sum_j beta3'(u - j) T[j, k(o)]
        gradient[d, e] = sum_o dI G_d o~_e            = d loss / d mat[:D] exactly, with the mask, the ranges and the fixed bins
                                                        held constant (the constant terms of d MI / d P vanish: sum_j beta3' = 0)
        c(o) = (omega / W) s^2 sum_j |beta3''(u - j)| |T[j, k(o)]|
        hessian[d (D+1) + e, d' (D+1) + e'] = sum_o c G_d G_d' o~_e o~_e'       the index order of gradient.reshape(P)

    The Hessian is a MAJORISER, not a Gauss-Newton matrix: the part of the true Hessian that goes through P is negative
    semi-definite (Cauchy-Schwarz: (d p_m)^2 / p_m <= sum_k (d P)^2 / P) and is dropped, the per-sample curvature beta3'' T is bounded
    term by term, and, as in every data term here, the second derivative of I is neglected.  It is the full matrix, both triangles
    from the same sum: exactly symmetric, positive semi-definite.  `hessian=False` computes none and the third item is None.
    `interpolation`, `bound`, `extrapolate`, `prefilter`, the batch broadcasting and the dtype and device rules as for
    `ssd_gauss_newton_affine`.  A plain loop:

        mat = torch.eye(D + 1, dtype=moving.dtype, device=moving.device)[:D]
        for _ in range(30):
            loss, g, H = mi_gauss_newton_affine(moving, fixed, mat, interpolation=3)
            step = torch.linalg.solve(H.double(), g.reshape(-1).double())
            mat = mat - step.reshape(D, D + 1).to(mat.dtype)

    On the GPU, D <= 3, float32 / float64, bins <= 64 and one order out of `backend.fused_mi_affine_orders` (measured,
    profiles/mi_affine.txt) run the fused kernels (csrc/mi_affine.hip: the histogram in 64-bit fixed point -- I, u and beta3 evaluated in
    double from the tensors' values, integer adds in LDS and across workgroups, exact in any order --, one workgroup per item for P, T and the loss in double, and the sums of
    `ssd_gauss_newton_affine` with T in LDS; nothing of size N is written; two calls give identical bits, and an item gives the same
    bits alone or inside a batch); everything else runs the composed form (`torch_kernels.mi_gauss_newton_affine_composed`: a dense
    lattice, `index_add_` into a float64 histogram and float64 contractions; 16-bit tensors compute in float32 and are rounded
    once; its histogram is not bit-reproducible on the GPU).  NOT differentiable: with grad mode on and an input that requires
    grad it raises RuntimeError (call it under torch.no_grad(), or detach)."""
    if backend.jitfields:
        raise RuntimeError('the jitfields backend is not part of the MI355X build')
    names = ['moving', 'fixed', 'mat'] + ([] if weight is None else ['weight'])
    tensors = [moving, fixed, mat] + ([] if weight is None else [weight])
    if not all(torch.is_tensor(t) and t.dtype.is_floating_point for t in tensors):
        raise ValueError('mi_gauss_newton_affine: `moving`, `fixed`, `mat` and `weight` must be floating point tensors')
    for n, t in zip(names, tensors):
        if t.dtype != mat.dtype or t.device != mat.device:
            raise ValueError('mi_gauss_newton_affine: `%s` must have the dtype and device of `mat`, got %s on %s and %s on %s'
                             % (n, t.dtype, t.device, mat.dtype, mat.device))
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        raise RuntimeError('mi_gauss_newton_affine is not differentiable: call it under torch.no_grad() or detach its inputs')
    _mi_options('mi_gauss_newton_affine', bins, moving_range, fixed_range)
    dim = mat.shape[-1] - 1 if mat.dim() >= 2 else 0
    if dim < 1 or mat.shape[-2] not in (dim, dim + 1) or fixed.dim() < dim + 1 or moving.dim() < dim + 1:
        raise ValueError('mi_gauss_newton_affine: `mat` (..., D or D+1, D+1) sets the number of spatial dimensions: `moving` '
                         '(..., 1, *inshape), `fixed` (..., 1, *shape), got %s, %s and %s'
                         % (list(mat.shape), list(moving.shape), list(fixed.shape)))
    shape = tuple(fixed.shape[-dim:])
    if weight is not None and (weight.dim() < dim or tuple(weight.shape[-dim:]) != shape):
        raise ValueError('mi_gauss_newton_affine: `weight` must have the spatial shape of `fixed`, got %s and %s'
                         % (list(weight.shape), list(fixed.shape)))
    if moving.shape[-dim - 1] != 1 or fixed.shape[-dim - 1] != 1:
        raise ValueError('mi_gauss_newton_affine: `moving` and `fixed` must have ONE channel, got %d and %d'
                         % (moving.shape[-dim - 1], fixed.shape[-dim - 1]))
    mat = mat[..., :dim, :]
    nb = [moving.dim() - dim - 1, fixed.dim() - dim - 1, mat.dim() - 2] + ([] if weight is None else [weight.dim() - dim])
    batch = ()
    for t, n in zip(tensors, nb):
        batch = tuple(expanded_shape(batch, tuple(t.shape[:n])))
    with torch.no_grad():
        if prefilter and _filters(interpolation, dim):
            moving = spline_coeff_nd(moving, interpolation=interpolation, bound=bound, dim=dim)
        m, f, a = (_fold_batch(t, n, batch) for t, n in zip((moving, fixed, mat), nb))
        w = None if weight is None else _fold_batch(weight, nb[3], batch)
        loss, gradient, hess, hist = ops.mi_gauss_newton_affine(m, f, a, w, *_options(bound, interpolation, extrapolate), bool(hessian),
                                                                bins, moving_range, fixed_range, bool(return_histogram))
    loss = loss.reshape(batch)
    gradient = gradient.reshape([*batch, dim, dim + 1])
    if hess is not None:
        hess = hess.reshape([*batch, *hess.shape[1:]])
    if return_histogram:
        return loss, gradient, hess, hist.reshape([*batch, bins, bins])
    return loss, gradient, hess


def mi_gauss_newton(moving, fixed, disp, weight=None, bins=32, moving_range=None, fixed_range=None, interpolation=1, bound='dct2',
                    extrapolate=True, prefilter=False, hessian='full', return_histogram=False):
    """The mutual-information data term of a Gauss-Newton registration step on a dense displacement field (an extension): minus
    the mutual information of the joint Parzen histogram of moving(id + disp) and fixed, its gradient with respect to `disp` and a
    per-voxel majoriser of the Hessian.  Invariant to the intensity scale of either image: the data term of the non-linear step
    of a multi-modal alignment, the companion of `mi_gauss_newton_affine`.

    moving (..., 1, *inshape), fixed (..., 1, *shape) -- ONE channel --, disp (..., *shape, D) voxel displacements on the lattice of
    `fixed`, weight None or (..., *shape), weight >= 0 (not checked) -> (loss (...), gradient (..., *shape, D), hessian
    (..., *shape, K) | None); with `return_histogram=True` also the joint histogram (..., bins, bins) as a fourth item.  The sample
    of lattice point o sits at x(o) = o + disp(o):

        I = grid_pull(moving, disp, displacement=True, ...),   G = grid_grad(moving, disp, displacement=True, ...),   J = fixed

    `bins`, `moving_range`, `fixed_range` and every formula from the in-view mask m, omega = weight m and W = sum_o omega over t_m,
    t_f, k(o), u(o), P, p_m, p_f, T, the loss and s to dI(o) and c(o) are those of `mi_gauss_newton_affine`.  The outputs are per
    voxel:

        gradient[o, d] = dI(o) G_d(o)            = d loss / d disp[o, d] exactly, with the mask, the ranges and the fixed bins held
                                                   constant
        hessian[o, k]  = c(o) G_d(o) G_e(o)      a majoriser (the argument of `mi_gauss_newton_affine`), positive semi-definite for
                                                   weight >= 0

    `hessian='full'`: K = D (D + 1) / 2, the diagonal first and then the upper triangle row by row -- what
    `regulariser_solve(hessian=...)` takes; 'diagonal': K = D; None: no Hessian is computed and the third item is None.
    Out-of-view samples under `extrapolate=False` are excluded from the histogram; their gradient and Hessian are zero.  W <= 0:
    every output is zero.  `interpolation`, `bound`, `extrapolate`, `prefilter`, the batch broadcasting and the dtype and device
    rules as for `ssd_gauss_newton`.  A plain loop, lam a membrane weight:

        disp = torch.zeros(*shape, D)
        for _ in range(12):
            loss, g, H = mi_gauss_newton(moving, fixed, disp, bins=16)
            g += regulariser(disp, membrane=lam, bound='dct2')
            disp -= regulariser_solve(g, H, membrane=lam, bound='dct2')

    On the GPU, D <= 3, float32 / float64, bins <= 64 and one order out of `backend.fused_mi_orders` (measured, profiles/mi.txt) run
    the fused kernels (csrc/mi.hip: the histogram in 64-bit fixed point -- I, u and beta3 evaluated in double from the tensors'
    values, integer adds in LDS and across workgroups, exact in any order --, one workgroup per item for P, T and the loss in double,
    and one thread per sample for the two fields with T in LDS; two calls give identical bits, and an item gives the same bits alone
    or inside a batch); everything else runs the composed form (`torch_kernels.mi_gauss_newton_composed`; 16-bit tensors compute in
    float32 and are rounded once; its histogram is not bit-reproducible on the GPU).  NOT differentiable: with grad mode on and an
    input that requires grad it raises RuntimeError (call it under torch.no_grad(), or detach)."""
    dim, nb, batch = _data_term_operands('mi_gauss_newton', moving, fixed, disp, weight, hessian)
    _mi_options('mi_gauss_newton', bins, moving_range, fixed_range)
    if moving.shape[-dim - 1] != 1:                  # (`fixed` has the channels of `moving`: checked above)
        raise ValueError('mi_gauss_newton: `moving` and `fixed` must have ONE channel, got %d and %d'
                         % (moving.shape[-dim - 1], fixed.shape[-dim - 1]))
    with torch.no_grad():
        if prefilter and _filters(interpolation, dim):
            moving = spline_coeff_nd(moving, interpolation=interpolation, bound=bound, dim=dim)
        m, f, u = (_fold_batch(t, n, batch) for t, n in zip((moving, fixed, disp), nb))
        w = None if weight is None else _fold_batch(weight, nb[3], batch)
        loss, gradient, hess, hist = ops.mi_gauss_newton(m, f, u, w, *_options(bound, interpolation, extrapolate), hessian, bins,
                                                         moving_range, fixed_range, bool(return_histogram))
    loss = loss.reshape(batch)
    gradient = gradient.reshape([*batch, *gradient.shape[1:]])
    if hess is not None:
        hess = hess.reshape([*batch, *hess.shape[1:]])
    if return_histogram:
        return loss, gradient, hess, hist.reshape([*batch, bins, bins])
    return loss, gradient, hess


pull = grid_pull
push = grid_push
count = grid_count
