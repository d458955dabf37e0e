"""Differentiable operators (autograd boundary).

Counterpart of the reference's `interpol/autograd.py:157-333`: six
`torch.autograd.Function`s with the same `apply(...)` signatures, the same
alias handling (`bound_to_nitorch` / `inter_to_nitorch`), float32 up-casting
under CUDA autocast, and `requires_grad`-driven skipping in backward.  The
forward and backward bodies call the fused HIP operators of `ops.py`.
`AffinePull` / `AffinePush` / `AffineCount` (an extension) are pull / push /
count on an `AffineGrid` whose matrix is an input with a gradient.
`Compose` (an extension) is the composition of two displacement fields;
`Jacobian` / `JacDet` (an extension) are the Jacobian of id + a displacement
field at the lattice points and its determinant; `Regulariser` /
`RegulariserEnergy` (an extension) are the absolute / membrane / bending
penalty of a displacement field as a matrix-vector product and as an energy.
"""
import torch

from . import ops
from .coeff import _spline_coeff, _spline_coeff_nd
from .codes import bound_to_code, order_to_code, pad_codes
from .torch_kernels import SLIDING
from .sepgrid import SeparableGrid, AffineGrid, LazyGrid
from .utils import affine_grid, identity_grid

try:                                    # torch >= 2.4
    from torch.amp import custom_fwd, custom_bwd
    _fwd32 = custom_fwd(device_type='cuda', cast_inputs=torch.float32)
    _fwd = custom_fwd(device_type='cuda')
    _bwd = custom_bwd(device_type='cuda')
except ImportError:                     # pragma: no cover
    from torch.cuda.amp import custom_fwd, custom_bwd
    _fwd32 = custom_fwd(cast_inputs=torch.float32)
    _fwd = custom_fwd
    _bwd = custom_bwd


def _as_list(x):
    return list(x) if isinstance(x, (list, tuple)) else [x]


def _save(ctx, input, grid):
    """save_for_backward with a constant SeparableGrid kept as a plain attribute."""
    if isinstance(grid, LazyGrid):
        ctx.sep = grid
        ctx.save_for_backward(input)
    else:
        ctx.sep = None
        ctx.save_for_backward(input, grid)


def _saved(ctx):
    if ctx.sep is not None:
        return ctx.saved_tensors[0], ctx.sep
    return ctx.saved_tensors


def _extra(displacement):
    """Optional trailing `displacement` argument of the sampling Functions (an extension: the
    reference's `apply` signatures stay valid).  -> (flag, number of extra inputs)."""
    return (bool(displacement[0]) if displacement else False), len(displacement)


def _higher_order():
    """Inside a `backward`: is a graph being recorded (create_graph=True)?  Then the gradients must
    themselves be differentiable: the backward is composed from the Functions of this module (as the
    reference's backward is composed from differentiable torch ops, pushpull.py:237-325) instead of
    calling the fused kernels, whose outputs carry no graph."""
    return torch.is_grad_enabled()


def _extra_args(ctx):
    return (ctx.disp,) if ctx.nextra else ()


def _options(bound, interpolation, extrapolate):
    return ([bound_to_code(b) for b in _as_list(bound)],
            [order_to_code(o) for o in _as_list(interpolation)],
            int(extrapolate))


class GridPull(torch.autograd.Function):
    """reference interpol/autograd.py:157-184"""

    @staticmethod
    @_fwd32
    def forward(ctx, input, grid, interpolation, bound, extrapolate, *displacement):
        opt = _options(bound, interpolation, extrapolate)
        ctx.disp, ctx.nextra = _extra(displacement)
        output = ops.grid_pull(input, grid, *opt, displacement=ctx.disp)
        ctx.opt = opt
        _save(ctx, input, grid)
        return output

    @staticmethod
    @_bwd
    def backward(ctx, grad):
        input, grid = _saved(ctx)
        if _higher_order():
            # pull backward = push of the gradient & contraction of grid_grad (pushpull.py:237-258)
            bound, interpolation, extrapolate = ctx.opt
            grad_input = grad_grid = None
            if ctx.needs_input_grad[0]:
                grad_input = GridPush.apply(grad, grid, list(input.shape[2:]), interpolation, bound, extrapolate, *_extra_args(ctx))
            if ctx.needs_input_grad[1]:
                grad_grid = (GridGrad.apply(input, grid, interpolation, bound, extrapolate, *_extra_args(ctx)) * grad.unsqueeze(-1)).sum(1)
            return (grad_input, grad_grid, None, None, None) + (None,) * ctx.nextra
        grad_input, grad_grid = ops.grid_pull_backward(
            grad, input, grid, *ctx.opt,
            need_inp=ctx.needs_input_grad[0], need_grid=ctx.needs_input_grad[1], displacement=ctx.disp)
        return (grad_input, grad_grid, None, None, None) + (None,) * ctx.nextra


class GridPush(torch.autograd.Function):
    """reference interpol/autograd.py:187-214"""

    @staticmethod
    @_fwd32
    def forward(ctx, input, grid, shape, interpolation, bound, extrapolate, *displacement):
        opt = _options(bound, interpolation, extrapolate)
        ctx.disp, ctx.nextra = _extra(displacement)
        output = ops.grid_push(input, grid, shape, *opt, displacement=ctx.disp)
        ctx.opt = opt
        _save(ctx, input, grid)
        return output

    @staticmethod
    @_bwd
    def backward(ctx, grad):
        input, grid = _saved(ctx)
        if _higher_order():
            # push backward = pull of the gradient & contraction of its grid_grad (pushpull.py:262-292)
            bound, interpolation, extrapolate = ctx.opt
            grad_input = grad_grid = None
            if ctx.needs_input_grad[0]:
                grad_input = GridPull.apply(grad, grid, interpolation, bound, extrapolate, *_extra_args(ctx))
            if ctx.needs_input_grad[1]:
                grad_grid = (GridGrad.apply(grad, grid, interpolation, bound, extrapolate, *_extra_args(ctx)) * input.unsqueeze(-1)).sum(1)
            return (grad_input, grad_grid, None, None, None, None) + (None,) * ctx.nextra
        grad_input, grad_grid = ops.grid_push_backward(
            grad, input, grid, *ctx.opt,
            need_inp=ctx.needs_input_grad[0], need_grid=ctx.needs_input_grad[1], displacement=ctx.disp)
        return (grad_input, grad_grid, None, None, None, None) + (None,) * ctx.nextra


class GridCount(torch.autograd.Function):
    """reference interpol/autograd.py:217-245"""

    @staticmethod
    @_fwd32
    def forward(ctx, grid, shape, interpolation, bound, extrapolate, *displacement):
        opt = _options(bound, interpolation, extrapolate)
        ctx.disp, ctx.nextra = _extra(displacement)
        output = ops.grid_count(grid, shape, *opt, displacement=ctx.disp)
        ctx.opt = opt
        ctx.save_for_backward(grid)
        return output

    @staticmethod
    @_bwd
    def backward(ctx, grad):
        grid, = ctx.saved_tensors
        grad_grid = None
        if ctx.needs_input_grad[0] and _higher_order():
            # count backward = grid_grad of the gradient, summed over its channel (pushpull.py:296-325)
            bound, interpolation, extrapolate = ctx.opt
            grad_grid = GridGrad.apply(grad, grid, interpolation, bound, extrapolate, *_extra_args(ctx)).sum(1)
        elif ctx.needs_input_grad[0]:
            grad_grid = ops.grid_count_backward(grad, grid, *ctx.opt, need_grid=True, displacement=ctx.disp)
        return (grad_grid, None, None, None, None) + (None,) * ctx.nextra


# ---------------------------------------------------------------------------
# Affine lattices with a learnable matrix: `mat` (D, D+1) is a real tensor input, the lattice AffineGrid(mat, shape) is
# evaluated inside the kernels in both directions.  forward = today's operator on the constant lattice; backward = the
# existing fused backward for the image (no grid gradient) and the on-chip reduction of csrc/affine_grad.hip for `mat`.
# ---------------------------------------------------------------------------
def _index_moments(grad_grid, shape):
    """(B,*shape,D) grid gradient -> (D, D+1): sum_b sum_o g_d(b,o) [o | 1]_e, the chain rule through affine_grid (api.py:534-572)
    written with torch ops (the create_graph route: differentiable in grad_grid)."""
    dim = len(shape)
    o = identity_grid(shape, dtype=grad_grid.dtype, device=grad_grid.device).reshape(-1, dim)
    o = torch.cat([o, o.new_ones([o.shape[0], 1])], 1)
    return grad_grid.sum(0).reshape(-1, dim).t() @ o


class AffinePull(torch.autograd.Function):
    """grid_pull(input, AffineGrid(mat, shape)): (B,C,*in), (D,D+1) -> (B,C,*shape)"""

    @staticmethod
    @_fwd32
    def forward(ctx, input, mat, shape, interpolation, bound, extrapolate):
        ctx.opt = _options(bound, interpolation, extrapolate)
        ctx.shape = [int(n) for n in shape]
        ctx.save_for_backward(input, mat)
        return ops.grid_pull(input, AffineGrid(mat.detach(), ctx.shape), *ctx.opt)

    @staticmethod
    @_bwd
    def backward(ctx, grad):
        input, mat = ctx.saved_tensors
        bound, interpolation, extrapolate = ctx.opt
        grad_input = grad_mat = None
        if _higher_order():
            # composed from the differentiable Functions on the dense lattice, like GridPull.backward
            grid = affine_grid(mat, ctx.shape)[None]
            if ctx.needs_input_grad[0]:
                grad_input = GridPush.apply(grad, grid, list(input.shape[2:]), interpolation, bound, extrapolate)
            if ctx.needs_input_grad[1]:
                grad_grid = (GridGrad.apply(input, grid, interpolation, bound, extrapolate) * grad.unsqueeze(-1)).sum(1)
                grad_mat = _index_moments(grad_grid, ctx.shape).to(mat.dtype)
            return grad_input, grad_mat, None, None, None, None
        lattice = AffineGrid(mat.detach(), ctx.shape)
        if ctx.needs_input_grad[0]:
            grad_input = ops.grid_pull_backward(grad, input, lattice, *ctx.opt, need_inp=True, need_grid=False)[0]
        if ctx.needs_input_grad[1]:
            grad_mat = ops.grid_pull_backward_affine(grad, input, lattice, *ctx.opt).to(mat.dtype)
        return grad_input, grad_mat, None, None, None, None


class AffinePush(torch.autograd.Function):
    """grid_push(input, AffineGrid(mat, inshape), shape): (B,C,*inshape), (D,D+1) -> (B,C,*shape).
    `inshape` is the lattice's own shape, as in AffinePull / AffineCount: the operator checks it against the image
    exactly as it does for a constant lattice."""

    @staticmethod
    @_fwd32
    def forward(ctx, input, mat, inshape, shape, interpolation, bound, extrapolate):
        ctx.opt = _options(bound, interpolation, extrapolate)
        ctx.inshape = [int(n) for n in inshape]
        ctx.save_for_backward(input, mat)
        return ops.grid_push(input, AffineGrid(mat.detach(), ctx.inshape), shape, *ctx.opt)

    @staticmethod
    @_bwd
    def backward(ctx, grad):
        input, mat = ctx.saved_tensors
        bound, interpolation, extrapolate = ctx.opt
        grad_input = grad_mat = None
        if _higher_order():
            grid = affine_grid(mat, ctx.inshape)[None]
            if ctx.needs_input_grad[0]:
                grad_input = GridPull.apply(grad, grid, interpolation, bound, extrapolate)
            if ctx.needs_input_grad[1]:
                grad_grid = (GridGrad.apply(grad, grid, interpolation, bound, extrapolate) * input.unsqueeze(-1)).sum(1)
                grad_mat = _index_moments(grad_grid, ctx.inshape).to(mat.dtype)
            return grad_input, grad_mat, None, None, None, None, None
        lattice = AffineGrid(mat.detach(), ctx.inshape)
        if ctx.needs_input_grad[0]:
            grad_input = ops.grid_push_backward(grad, input, lattice, *ctx.opt, need_inp=True, need_grid=False)[0]
        if ctx.needs_input_grad[1]:
            grad_mat = ops.grid_push_backward_affine(grad, input, lattice, *ctx.opt).to(mat.dtype)
        return grad_input, grad_mat, None, None, None, None, None


class AffineCount(torch.autograd.Function):
    """grid_count(AffineGrid(mat, inshape), shape): (D,D+1) -> (1,1,*shape)"""

    @staticmethod
    @_fwd32
    def forward(ctx, mat, inshape, shape, interpolation, bound, extrapolate):
        ctx.opt = _options(bound, interpolation, extrapolate)
        ctx.inshape = [int(n) for n in inshape]
        ctx.save_for_backward(mat)
        return ops.grid_count(AffineGrid(mat.detach(), ctx.inshape), shape, *ctx.opt)

    @staticmethod
    @_bwd
    def backward(ctx, grad):
        mat, = ctx.saved_tensors
        bound, interpolation, extrapolate = ctx.opt
        grad_mat = None
        if ctx.needs_input_grad[0] and _higher_order():
            grid = affine_grid(mat, ctx.inshape)[None]
            grad_grid = GridGrad.apply(grad, grid, interpolation, bound, extrapolate).sum(1)
            grad_mat = _index_moments(grad_grid, ctx.inshape).to(mat.dtype)
        elif ctx.needs_input_grad[0]:
            grad_mat = ops.grid_push_backward_affine(grad, None, AffineGrid(mat.detach(), ctx.inshape), *ctx.opt).to(mat.dtype)
        return grad_mat, None, None, None, None, None


class GridGrad(torch.autograd.Function):
    """reference interpol/autograd.py:248-277"""

    @staticmethod
    @_fwd32
    def forward(ctx, input, grid, interpolation, bound, extrapolate, *displacement):
        opt = _options(bound, interpolation, extrapolate)
        ctx.disp, ctx.nextra = _extra(displacement)
        output = ops.grid_grad(input, grid, *opt, displacement=ctx.disp)
        ctx.opt = opt
        _save(ctx, input, grid)
        return output

    @staticmethod
    @_bwd
    def backward(ctx, grad):
        input, grid = _saved(ctx)
        grad_input = grad_grid = None
        if _higher_order() and (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            # Third order and beyond (create_graph=True inside a double backward).  The reference's backward is plain torch and
            # differentiates on (pushpull.py:303-325); the fused kernels (pushgrad, hess) carry no graph, so here autograd itself
            # differentiates the differentiable restatement of grid_grad (torch_kernels.py: weights and their derivatives as torch
            # expressions of the coordinates, one gather per chunk) -- every order from here on, at PyTorch speed.
            from .torch_kernels import TorchKernels
            bound, interpolation, extrapolate = ctx.opt
            bound, interpolation = ops._codes(grid, bound, interpolation)
            wrt = [t for t, need in ((input, ctx.needs_input_grad[0]), (grid, ctx.needs_input_grad[1])) if need]
            with torch.enable_grad():
                out = TorchKernels.grad(input, grid, bound, interpolation, int(extrapolate), displacement=ctx.disp)
                got = list(torch.autograd.grad(out, wrt, grad.to(out.dtype), create_graph=True, allow_unused=True))
            if ctx.needs_input_grad[0]:
                grad_input = got.pop(0)
            if ctx.needs_input_grad[1]:
                grad_grid = got.pop(0)
            return (grad_input, grad_grid, None, None, None) + (None,) * ctx.nextra
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            grad_input, grad_grid = ops.grid_grad_backward(
                grad, input, grid, *ctx.opt,
                need_inp=ctx.needs_input_grad[0], need_grid=ctx.needs_input_grad[1], displacement=ctx.disp)
        return (grad_input, grad_grid, None, None, None) + (None,) * ctx.nextra


def _batch_sum(grad, like):
    """gradient of an input whose batch of 1 was broadcast"""
    if grad is not None and like.shape[0] == 1 and grad.shape[0] > 1:
        grad = grad.sum(0, keepdim=True)
    return grad


class Compose(torch.autograd.Function):
    """Composition of voxel displacement fields (an extension): left (B|1,*lshape,D), right (B|1,*oshape,D) ->
    right + pull(left, id + right), (B,*oshape,D), point by point in and out (csrc/compose.hip)."""

    @staticmethod
    @_fwd32
    def forward(ctx, left, right, interpolation, bound, extrapolate):
        ctx.opt = _options(bound, interpolation, extrapolate)
        ctx.save_for_backward(left, right)
        return ops.compose(left, right, *ctx.opt)

    @staticmethod
    @_bwd
    def backward(ctx, grad):
        left, right = ctx.saved_tensors
        need_left, need_right = ctx.needs_input_grad[:2]
        grad_left = grad_right = None
        if _higher_order() and (need_left or need_right):
            # the gradients of the composed expression over GridPull, written with the differentiable Functions like
            # GridPull.backward: push of the gradient, contraction of grid_grad (pushpull.py:237-258).  A broadcast batch is
            # expanded here, so that autograd sums over it.
            bound, interpolation, extrapolate = ctx.opt
            B = grad.shape[0]
            l = left.expand(B, *left.shape[1:]).movedim(-1, 1)
            r = right.expand(B, *right.shape[1:])
            g = grad.movedim(-1, 1)
            if need_left:
                grad_left = GridPush.apply(g, r, list(left.shape[1:-1]), interpolation, bound, extrapolate, True).movedim(1, -1)
            if need_right:
                grad_right = grad + (GridGrad.apply(l, r, interpolation, bound, extrapolate, True) * g.unsqueeze(-1)).sum(1)
            return _batch_sum(grad_left, left), _batch_sum(grad_right, right), None, None, None
        if need_left or need_right:
            grad_left, grad_right = ops.compose_backward(grad, left, right, *ctx.opt, need_left=need_left, need_right=need_right)
            grad_left, grad_right = _batch_sum(grad_left, left), _batch_sum(grad_right, right)
        return grad_left, grad_right, None, None, None


def _lattice_graph(fn, disp, grad, bound, interpolation, *extra):
    """Backward of Jacobian / JacDet while a graph is recorded: autograd differentiates the differentiable restatement
    (torch_kernels.py, as GridGrad does from the third order on), so the result carries a graph in `grad` and in `disp`."""
    from .torch_kernels import TorchKernels
    bound, interpolation = ops._codes(disp, bound, interpolation)
    with torch.enable_grad():
        out = fn(TorchKernels, disp, bound, interpolation, *extra)
        return torch.autograd.grad(out, disp, grad.to(out.dtype), create_graph=True)[0]


class Jacobian(torch.autograd.Function):
    """Jacobian of id + disp at the lattice points (an extension): disp (B,*shape,D) -> (B,*shape,D,D) (csrc/jacobian.hip)."""

    @staticmethod
    @_fwd32
    def forward(ctx, disp, interpolation, bound, add_identity):
        ctx.opt = _options(bound, interpolation, 1)[:2]
        ctx.add_identity = bool(add_identity)
        ctx.save_for_backward(disp)
        return ops.jacobian(disp, *ctx.opt, add_identity=ctx.add_identity)

    @staticmethod
    @_bwd
    def backward(ctx, grad):
        disp, = ctx.saved_tensors
        grad_disp = None
        if ctx.needs_input_grad[0] and _higher_order():
            from .torch_kernels import jacobian_composed
            grad_disp = _lattice_graph(jacobian_composed, disp, grad, *ctx.opt, ctx.add_identity)
        elif ctx.needs_input_grad[0]:
            grad_disp = ops.jacobian_backward(grad, *ctx.opt).to(disp.dtype)
        return grad_disp, None, None, None


class JacDet(torch.autograd.Function):
    """Determinant of the Jacobian of id + disp at the lattice points (an extension): disp (B,*shape,D) -> (B,*shape)."""

    @staticmethod
    @_fwd32
    def forward(ctx, disp, interpolation, bound):
        ctx.opt = _options(bound, interpolation, 1)[:2]
        ctx.save_for_backward(disp)
        return ops.jacdet(disp, *ctx.opt)

    @staticmethod
    @_bwd
    def backward(ctx, grad):
        disp, = ctx.saved_tensors
        grad_disp = None
        if ctx.needs_input_grad[0] and _higher_order():
            from .torch_kernels import jacdet_composed
            grad_disp = _lattice_graph(jacdet_composed, disp, grad, *ctx.opt)
        elif ctx.needs_input_grad[0]:
            grad_disp = ops.jacdet_backward(grad, disp, *ctx.opt)
        return grad_disp, None, None


def regulariser_bound_codes(bound, dim):
    """`bound` of the regulariser functions -> D codes: those of every other function, and 'sliding' (7), the one
    per-component bound -- known to the regulariser functions only (codes.bound_to_code does not take it)"""
    return pad_codes([SLIDING if (isinstance(b, str) and b.lower() == 'sliding') or (type(b) is int and b == SLIDING)
                      else bound_to_code(b) for b in _as_list(bound)], dim)


def _regulariser_options(field, weights, voxel_size, bound):
    dim = field.shape[-1]
    return tuple(float(w) for w in weights), tuple(float(h) for h in voxel_size), regulariser_bound_codes(bound, dim)


def _regulariser_symmetric(bound, weights=(0., 0., 0.)):
    """Is L symmetric?  bound: D codes; weights: three or five.  zero, dft and sliding in every dimension; without elastic
    weights (shears, div: weights[3:]) also dct2 and dst2 (replicate, dct1 and dst1 never are; with shears + div > 0 one
    bound for every component is not either, but for zero and dft)"""
    ok = (0, 6, SLIDING) if any(weights[3:]) else (0, 3, 5, 6, SLIDING)
    return all(b in ok for b in bound)


def _regulariser_graph(fn, wrt, grad, weights, voxel_size, bound):
    """grad * d fn / d wrt through the composed form (torch_kernels.py), which autograd differentiates for every bound; under
    create_graph=True the result carries a graph in `grad` (and in `wrt`, where fn is not linear)."""
    from . import torch_kernels
    with torch.enable_grad():
        out = getattr(torch_kernels, fn)(wrt, weights, voxel_size, bound)
        return torch.autograd.grad(out, wrt, grad.to(out.dtype), create_graph=_higher_order())[0]


class Regulariser(torch.autograd.Function):
    """L v of a displacement field (an extension): field (B,*shape,D) -> (B,*shape,D) (csrc/regulariser.hip).  L is linear: the
    backward is L^T grad -- where L is symmetric (zero, dft, sliding in every dim; without elastic weights also dct2, dst2) this very Function again, so it differentiates
    any number of times on the fused kernel; else the transpose of the composed form, against a dummy input."""

    @staticmethod
    @_fwd32
    def forward(ctx, field, weights, voxel_size, bound):
        ctx.opt = _regulariser_options(field, weights, voxel_size, bound)
        return ops.regulariser(field, *ctx.opt)

    @staticmethod
    @_bwd
    def backward(ctx, grad):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        if _regulariser_symmetric(ctx.opt[2], ctx.opt[0]):
            return Regulariser.apply(grad, *ctx.opt), None, None, None
        dummy = torch.zeros_like(grad, requires_grad=True)
        return _regulariser_graph("regulariser_composed", dummy, grad, *ctx.opt), None, None, None


class RegulariserEnergy(torch.autograd.Function):
    """0.5 <v, L v> per batch item (an extension): field (B,*shape,D) -> (B).  Backward: grad * 0.5 (L + L^T) v -- grad * L v by
    `Regulariser` where L is symmetric, else through the composed form."""

    @staticmethod
    @_fwd32
    def forward(ctx, field, weights, voxel_size, bound):
        ctx.opt = _regulariser_options(field, weights, voxel_size, bound)
        ctx.save_for_backward(field)
        return ops.regulariser_energy(field, *ctx.opt)

    @staticmethod
    @_bwd
    def backward(ctx, grad):
        field, = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        if _regulariser_symmetric(ctx.opt[2], ctx.opt[0]):
            g = grad.reshape([-1] + [1] * (field.dim() - 1)).to(field.dtype) * Regulariser.apply(field, *ctx.opt)
            return g, None, None, None
        wrt = field if _higher_order() else field.detach().requires_grad_()
        return _regulariser_graph("regulariser_energy_composed", wrt, grad, *ctx.opt).to(field.dtype), None, None, None


class SplineCoeff(torch.autograd.Function):
    """reference interpol/autograd.py:280-305"""

    @staticmethod
    @_fwd
    def forward(ctx, input, bound, interpolation, dim, inplace):
        bound = bound_to_code(_as_list(bound)[0])
        interpolation = order_to_code(_as_list(interpolation)[0])
        ctx.opt = (bound, interpolation, dim)
        return _spline_coeff(input, bound, interpolation, dim, inplace)

    @staticmethod
    @_bwd
    def backward(ctx, grad):
        # the filter is symmetric: backward == forward (autograd.py:300-305)
        if _higher_order():
            return SplineCoeff.apply(grad, *ctx.opt, False), None, None, None, None
        return _spline_coeff(grad, *ctx.opt, inplace=False), None, None, None, None


class SplineCoeffND(torch.autograd.Function):
    """reference interpol/autograd.py:308-333"""

    @staticmethod
    @_fwd
    def forward(ctx, input, bound, interpolation, dim, inplace):
        bound = [bound_to_code(b) for b in _as_list(bound)]
        interpolation = [order_to_code(o) for o in _as_list(interpolation)]
        ctx.opt = (bound, interpolation, dim)
        return _spline_coeff_nd(input, bound, interpolation, dim, inplace)

    @staticmethod
    @_bwd
    def backward(ctx, grad):
        if _higher_order():
            return SplineCoeffND.apply(grad, *ctx.opt, False), None, None, None, None
        return _spline_coeff_nd(grad, *ctx.opt, inplace=False), None, None, None, None
