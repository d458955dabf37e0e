"""Operator seam: non-differentiable forward / backward operators.

Same functions, argument order and tensor layouts as the reference's
`interpol/pushpull.py` (grid_pull 35-66, grid_push 70-102, grid_count 106-142,
grid_grad 146-172, grid_pushgrad 176-203, grid_hess 207-233 and the four
`*_backward` compositions 237-325):

    inp  : (B, C, *spatial_in)      grid : (B, *spatial_out, D)
    bound / interpolation : lists of int codes, padded/truncated to D
    extrapolate : 0 | 1 | 2

but every operator is ONE fused HIP kernel launch (see `csrc/`) instead of
(order+1)^D passes of gather/scatter + broadcast multiplies, and the backward
operators are fused too (no (B,C,N,D) temporary).

`use_kernels(table)` swaps the kernel table; it exists for the CPU-side tests
of the host logic (shape conventions, autograd wiring) and is never used by the
product path, whose default table is the HIP library.
"""
import contextlib

import torch

from . import _hip
from .codes import pad_codes


def _dflag(displacement):
    return _hip.FLAG_DISPLACEMENT if displacement else 0


def _kw(displacement):
    """extra kernel-table keywords (tables that predate the flag are still callable without it)"""
    return {"displacement": True} if displacement else {}


class _HipKernels:
    """Default kernel table: the gfx950 library behind the C-ABI."""

    @staticmethod
    def pull(inp, grid, bound, order, extrapolate, displacement=False):
        return _hip.gather("pull", inp, grid, bound, order, extrapolate, flags=_dflag(displacement))

    @staticmethod
    def grad(inp, grid, bound, order, extrapolate, displacement=False):
        return _hip.gather("grad", inp, grid, bound, order, extrapolate, flags=_dflag(displacement))

    @staticmethod
    def hess(inp, grid, bound, order, extrapolate, displacement=False):
        return _hip.gather("hess", inp, grid, bound, order, extrapolate, flags=_dflag(displacement))

    @staticmethod
    def push(inp, grid, shape, bound, order, extrapolate, displacement=False):
        if shape is not None and _HipKernels.expanding(inp, grid, shape, False, order):
            return _hip.push_bricks(inp, grid, shape, bound, order, extrapolate, flags=_dflag(displacement))
        return _hip.scatter("push", inp, grid, shape, bound, order, extrapolate, flags=_dflag(displacement))

    @staticmethod
    def count(grid, shape, bound, order, extrapolate, displacement=False):
        return _hip.scatter("count", None, grid, shape, bound, order, extrapolate, flags=_dflag(displacement))

    @staticmethod
    def pushgrad(inp, grid, shape, bound, order, extrapolate, displacement=False):
        return _hip.scatter("pushgrad", inp, grid, shape, bound, order, extrapolate, flags=_dflag(displacement))

    @staticmethod
    def push_shared_(out, inp, grid, bound, order, extrapolate, with_count=False):
        """out (1,C,*shape) += sum over the batch of push(inp, grid); count when inp is None;
        with_count: out has C + 1 channels, the last one accumulates the count in the same pass."""
        op = "count" if inp is None else "push"
        shape = list(out.shape[2:])
        # Round 5: the batch items that share a target share its bricks too (csrc/push_owner.hip: BrickGrid::item = 0) -- once all
        # the sources together bring an EIGHTH of a sample per target voxel (dense_when_merged; BASELINE config 4: 64 sources of 128^3
        # into 512^3 bring a full one) the owner-computes organisation serves the call like a dense one (the probe of the call sends
        # it there): no atomics.  It needs ~22 B of workspace per sample over all sources: where that is denied the call goes on to
        # the organisations below (the target-stationary bricks first) instead of straight to the tiles.
        if _HipKernels.dense_when_merged(grid, shape, order):
            r = _hip.scatter(op, inp, grid, shape, bound, order, extrapolate,
                             flags=_hip.FLAG_ACCUMULATE, out=out, shared=True, with_count=with_count, need_workspace=True)
            if r is not None:
                return r
        if _HipKernels.expanding(inp, grid, shape, with_count, order):
            return _hip.push_bricks(inp, grid, shape, bound, order, extrapolate, flags=_hip.FLAG_ACCUMULATE, out=out,
                                    shared=True, with_count=with_count)
        return _hip.scatter(op, inp, grid, shape, bound, order, extrapolate,
                            flags=_hip.FLAG_ACCUMULATE, out=out, shared=True, with_count=with_count)

    @staticmethod
    def dense_when_merged(grid, shape, order):
        """Shared target: do the samples of ALL batch items make the owner-computes bricks worthwhile (3-D, one order 2..3)?"""
        from . import backend
        if backend.rough_deformations is False or backend.want_exact_scatter():
            return False
        if grid.shape[-1] != 3 or len(shape) != 3 or order is None or len(set(order)) != 1 or order[0] not in (2, 3):
            return False
        nsamp = int(grid.shape[0])
        for n in grid.shape[1:-1]:
            nsamp *= int(n)
        nvox = 1
        for n in shape:
            nvox *= int(n)
        return 8 * nsamp >= nvox

    @staticmethod
    def expanding(inp, grid, shape, with_count, order=None):
        """Is the target-stationary scheme (interpol_push_bricks) the better one?  Yes when the
        target has many more voxels than there are samples per item: neighbouring samples then own
        disjoint target voxels and a sample-stationary tile has nothing to merge."""
        if inp is None or not _hip.bricks_applicable(inp, grid, with_count, order):
            return False
        nsamp = 1
        for n in grid.shape[1:-1]:
            nsamp *= int(n)
        nvox = 1
        for n in shape:
            nvox *= int(n)
        return nvox >= 8 * nsamp

    @staticmethod
    def push_count(inp, grid, shape, bound, order, extrapolate, displacement=False):
        if shape is not None and _HipKernels.expanding(inp, grid, shape, True, order):
            return _hip.push_bricks(inp, grid, shape, bound, order, extrapolate, flags=_dflag(displacement), with_count=True)
        return _hip.scatter("push", inp, grid, shape, bound, order, extrapolate, flags=_dflag(displacement), with_count=True)

    @staticmethod
    def pull_backward(grad, inp, grid, bound, order, extrapolate, need_inp, need_grid, displacement=False):
        return _hip.pull_backward(grad, inp, grid, bound, order, extrapolate, need_inp, need_grid, flags=_dflag(displacement))

    @staticmethod
    def push_backward(grad, inp, grid, bound, order, extrapolate, need_inp, need_grid, displacement=False):
        return _hip.push_backward(grad, inp, grid, bound, order, extrapolate, need_inp, need_grid, flags=_dflag(displacement))

    @staticmethod
    def count_backward(grad, grid, bound, order, extrapolate, displacement=False):
        return _hip.push_backward(grad, None, grid, bound, order, extrapolate, False, True, flags=_dflag(displacement))[1]

    @staticmethod
    def affine_pull_backward(grad, inp, lattice, bound, order, extrapolate):
        return _hip.affine_pull_backward(grad, inp, lattice, bound, order, extrapolate)

    @staticmethod
    def affine_push_backward(grad, inp, lattice, bound, order, extrapolate):
        """inp None: backward of count"""
        return _hip.affine_push_backward(grad, inp, lattice, bound, order, extrapolate)

    @staticmethod
    def compose_fused(left, right, order):
        """The library takes these fields (_hip.compose_covered) AND the fused kernel is the faster route for this order
        (backend.fused_compose_orders: measured, profiles/compose.txt)."""
        from . import backend
        return _hip.compose_covered(left, right, order) and int(order[0]) in backend.fused_compose_orders

    @staticmethod
    def compose(left, right, bound, order, extrapolate, out=None):
        """right + pull(left, id + right), point by point: the fused kernel (csrc/compose.hip) where it applies, else composed
        from pull.  `out` may be `right`, never `left`."""
        if _HipKernels.compose_fused(left, right, order):
            return _hip.compose(left, right, bound, order, extrapolate, out=out)
        from .torch_kernels import composed
        res = composed(_HipKernels, left, right, bound, order, extrapolate)
        return res if out is None else out.copy_(res)

    @staticmethod
    def compose_backward(grad, left, right, bound, order, extrapolate, need_left, need_right):
        """-> (grad_left | None, grad_right | None), one per batch item of `grad`.  grad_right: the fused kernel; grad_left: the
        tuned push of `grad` along `right` (a scatter: it keeps its organisations, at the price of two layout copies)."""
        if not (_HipKernels.compose_fused(left, right, order) and grad.dtype == right.dtype):
            from .torch_kernels import composed_backward
            return composed_backward(_HipKernels, grad, left, right, bound, order, extrapolate, need_left, need_right)
        gl = gr = None
        if need_right:
            gr = _hip.compose_backward_right(grad, left, right, bound, order, extrapolate)
        if need_left:
            gl = _HipKernels.push(grad.movedim(-1, 1), right, list(left.shape[1:-1]), bound, order, extrapolate,
                                  displacement=True).movedim(1, -1)
        return gl, gr

    @staticmethod
    def jacobian_fused(disp, order):
        """The library takes this field (_hip.jacobian_covered) AND `backend.fused_jacobian_orders` routes this order to the fused
        kernels (measured, profiles/jacobian.txt)."""
        from . import backend
        return _hip.jacobian_covered(disp, order) and int(order[0]) in backend.fused_jacobian_orders

    @staticmethod
    def jacobian(disp, bound, order, add_identity=True):
        """Jacobian of id + disp at the lattice points, point by point: the fused kernel (csrc/jacobian.hip) where it applies, else
        composed from grad."""
        if _HipKernels.jacobian_fused(disp, order):
            return _hip.jacobian(disp, bound, order, det_only=False, add_identity=add_identity)
        from .torch_kernels import jacobian_composed
        return jacobian_composed(_HipKernels, disp, bound, order, add_identity)

    @staticmethod
    def jacdet(disp, bound, order):
        if _HipKernels.jacobian_fused(disp, order):
            return _hip.jacobian(disp, bound, order, det_only=True)
        from .torch_kernels import jacdet_composed
        return jacdet_composed(_HipKernels, disp, bound, order)

    @staticmethod
    def jacobian_backward(grad, bound, order):
        """grad (B,*shape,D,D) -> (B,*shape,D): no kernel of its own, the pushgrad of the gradient along a zero displacement"""
        from .torch_kernels import jacobian_backward_composed
        return jacobian_backward_composed(_HipKernels, grad, bound, order)

    @staticmethod
    def jacdet_backward(grad, disp, bound, order):
        """grad (B,*shape) -> (B,*shape,D).  Fused: one kernel recomputes J, writes grad * cofactor(J) as (B,D,*shape,D), and the
        tuned pushgrad takes it along a zero displacement of batch 1 (the scatter broadcasts it: batch stride 0)."""
        if not (_HipKernels.jacobian_fused(disp, order) and grad.dtype == disp.dtype):
            from .torch_kernels import jacdet_backward_composed
            return jacdet_backward_composed(_HipKernels, grad, disp, bound, order)
        G = _hip.jacdet_backward_field(grad, disp, bound, order)
        zero = disp.new_zeros([1, *disp.shape[1:]])
        return _HipKernels.pushgrad(G, zero, list(disp.shape[1:-1]), bound, order, 1, displacement=True).movedim(1, -1)

    @staticmethod
    def regulariser_fused(field):
        """The library takes this field (_hip.regulariser_covered) AND `backend.fused_regulariser` routes it to the fused kernels
        (measured, profiles/regulariser.txt)."""
        from . import backend
        return bool(backend.fused_regulariser) and _hip.regulariser_covered(field)

    @staticmethod
    def regulariser(field, weights, voxel_size, bound):
        """L field, point by point: the fused kernel (csrc/regulariser.hip) where it applies, else the composed form."""
        if _HipKernels.regulariser_fused(field):
            return _hip.regulariser(field, weights, voxel_size, bound)
        from .torch_kernels import regulariser_composed
        return regulariser_composed(field, weights, voxel_size, bound)

    @staticmethod
    def regulariser_energy(field, weights, voxel_size, bound):
        if _HipKernels.regulariser_fused(field):
            return _hip.regulariser_energy(field, weights, voxel_size, bound)
        from .torch_kernels import regulariser_energy_composed
        return regulariser_energy_composed(field, weights, voxel_size, bound)

    @staticmethod
    def regulariser_solve_fused(gradient, hessian):
        """The library takes these (_hip.regulariser_solve_covered) AND `backend.fused_regulariser_solve` routes them to the fused
        kernels (measured, profiles/regulariser_solve.txt)."""
        from . import backend
        return bool(backend.fused_regulariser_solve) and _hip.regulariser_solve_covered(gradient, hessian)

    @staticmethod
    def regulariser_solve(gradient, hessian, weights, voxel_size, bound, max_iter, tolerance):
        """(x, iterations, residual): the fused kernels (csrc/regulariser_solve.hip) where they apply, else the composed form."""
        if _HipKernels.regulariser_solve_fused(gradient, hessian):
            x, info = _hip.regulariser_solve(gradient, hessian, weights, voxel_size, bound, max_iter, tolerance)
            return x, info[:, 0].to(torch.int64), info[:, 1]
        from .torch_kernels import regulariser_solve_composed
        return regulariser_solve_composed(gradient, hessian, weights, voxel_size, bound, max_iter, tolerance)

    @staticmethod
    def regulariser_multigrid_fused(gradient, hessian):
        """The library takes these (_hip.regulariser_solve_covered) AND `backend.fused_regulariser_multigrid` routes them to the
        fused V-cycle (csrc/regulariser_multigrid.hip; measured, profiles/multigrid.txt)."""
        from . import backend
        return bool(backend.fused_regulariser_multigrid) and _hip.regulariser_solve_covered(gradient, hessian)

    @staticmethod
    def regulariser_multigrid(gradient, hessian, weights, voxel_size, bound, max_iter, tolerance, smoothing):
        """(x, iterations, residual) with the V-cycle as preconditioner: the fused kernels where they apply, else the composed form."""
        if _HipKernels.regulariser_multigrid_fused(gradient, hessian):
            x, info = _hip.regulariser_multigrid_solve(gradient, hessian, weights, voxel_size, bound, max_iter, tolerance, smoothing)
            return x, info[:, 0].to(torch.int64), info[:, 1]
        from .torch_kernels import regulariser_multigrid_composed
        return regulariser_multigrid_composed(gradient, hessian, weights, voxel_size, bound, max_iter, tolerance, smoothing)

    @staticmethod
    def regulariser_vcycle(residual, hessian, weights, voxel_size, bound, smoothing):
        if _HipKernels.regulariser_multigrid_fused(residual, hessian):
            return _hip.regulariser_multigrid_cycle(residual, hessian, weights, voxel_size, bound, smoothing)
        from .torch_kernels import regulariser_vcycle_composed
        return regulariser_vcycle_composed(residual, hessian, weights, voxel_size, bound, smoothing)

    @staticmethod
    def ssd_fused(moving, fixed, disp, weight, order, hessian='full'):
        """The library takes these (_hip.ssd_covered) AND `backend.fused_ssd_orders` -- without a Hessian,
        `backend.fused_ssd_orders_without_hessian` -- routes this order to the fused kernel (measured, profiles/ssd.txt)."""
        from . import backend
        routed = set(backend.fused_ssd_orders)
        if hessian is None:                              # (a narrower list on top: `fused_ssd_orders = ()` switches everything off)
            routed &= set(backend.fused_ssd_orders_without_hessian)
        return _hip.ssd_covered(moving, fixed, disp, weight, order) and int(order[0]) in routed

    @staticmethod
    def ssd_gauss_newton(moving, fixed, disp, weight, bound, order, extrapolate, hessian):
        """(loss, gradient, hessian | None): the fused kernel (csrc/ssd.hip) where it applies, else the composed form."""
        if _HipKernels.ssd_fused(moving, fixed, disp, weight, order, hessian):
            return _hip.ssd(moving, fixed, disp, weight, bound, order, extrapolate, hessian)
        from .torch_kernels import ssd_gauss_newton_composed
        return ssd_gauss_newton_composed(moving, fixed, disp, weight, bound, order, extrapolate, hessian)

    @staticmethod
    def lcc_fused(moving, fixed, disp, weight, order, window):
        """The library takes these (_hip.lcc_covered) AND `backend.fused_lcc_orders` routes this order to the fused kernels
        (measured, profiles/lcc.txt)."""
        from . import backend
        return _hip.lcc_covered(moving, fixed, disp, weight, order, window) and int(order[0]) in backend.fused_lcc_orders

    @staticmethod
    def lcc_gauss_newton(moving, fixed, disp, weight, bound, order, extrapolate, hessian, window, eps):
        """(loss, gradient, hessian | None): the fused kernels (csrc/lcc.hip) where they apply, else the composed form."""
        if _HipKernels.lcc_fused(moving, fixed, disp, weight, order, window):
            return _hip.lcc(moving, fixed, disp, weight, bound, order, extrapolate, hessian, window, eps)
        from .torch_kernels import lcc_gauss_newton_composed
        return lcc_gauss_newton_composed(moving, fixed, disp, weight, bound, order, extrapolate, hessian, window, eps)

    @staticmethod
    def ssd_affine_fused(moving, fixed, mat, weight, order):
        """The library takes these (_hip.ssd_affine_covered) AND `backend.fused_ssd_affine_orders` routes this order to the fused
        kernel (measured, profiles/ssd_affine.txt)."""
        from . import backend
        return _hip.ssd_affine_covered(moving, fixed, mat, weight, order) and int(order[0]) in backend.fused_ssd_affine_orders

    @staticmethod
    def ssd_gauss_newton_affine(moving, fixed, mat, weight, bound, order, extrapolate, hessian):
        """(loss, gradient, hessian | None): the fused kernel (csrc/ssd_affine.hip) where it applies, else the composed form."""
        if _HipKernels.ssd_affine_fused(moving, fixed, mat, weight, order):
            return _hip.ssd_affine(moving, fixed, mat, weight, bound, order, extrapolate, hessian)
        from .torch_kernels import ssd_gauss_newton_affine_composed
        return ssd_gauss_newton_affine_composed(moving, fixed, mat, weight, bound, order, extrapolate, hessian)

    @staticmethod
    def lcc_affine_fused(moving, fixed, mat, weight, order, window):
        """The library takes these (_hip.lcc_affine_covered) AND `backend.fused_lcc_affine_orders` routes this order to the fused
        kernels (measured, profiles/lcc_affine.txt)."""
        from . import backend
        return _hip.lcc_affine_covered(moving, fixed, mat, weight, order, window) and int(order[0]) in backend.fused_lcc_affine_orders

    @staticmethod
    def lcc_gauss_newton_affine(moving, fixed, mat, weight, bound, order, extrapolate, hessian, window, eps):
        """(loss, gradient, hessian | None): the fused kernels (csrc/lcc_affine.hip) where they apply, else the composed form."""
        if _HipKernels.lcc_affine_fused(moving, fixed, mat, weight, order, window):
            return _hip.lcc_affine(moving, fixed, mat, weight, bound, order, extrapolate, hessian, window, eps)
        from .torch_kernels import lcc_gauss_newton_affine_composed
        return lcc_gauss_newton_affine_composed(moving, fixed, mat, weight, bound, order, extrapolate, hessian, window, eps)

    @staticmethod
    def mi_affine_fused(moving, fixed, mat, weight, order, bins):
        """The library takes these (_hip.mi_affine_covered) AND `backend.fused_mi_affine_orders` routes this order to the fused
        kernels (measured, profiles/mi_affine.txt)."""
        from . import backend
        return _hip.mi_affine_covered(moving, fixed, mat, weight, order, bins) and int(order[0]) in backend.fused_mi_affine_orders

    @staticmethod
    def mi_gauss_newton_affine(moving, fixed, mat, weight, ranges, bound, order, extrapolate, hessian, bins, return_histogram):
        """(loss, gradient, hessian | None, histogram | None): the fused kernels (csrc/mi_affine.hip) where they apply, else the
        composed form."""
        if _HipKernels.mi_affine_fused(moving, fixed, mat, weight, order, bins):
            return _hip.mi_affine(moving, fixed, mat, weight, ranges, bound, order, extrapolate, hessian, bins, return_histogram)
        from .torch_kernels import mi_gauss_newton_affine_composed
        return mi_gauss_newton_affine_composed(moving, fixed, mat, weight, ranges, bound, order, extrapolate, hessian, bins,
                                               return_histogram)

    @staticmethod
    def mi_fused(moving, fixed, disp, weight, order, bins):
        """The library takes these (_hip.mi_covered) AND `backend.fused_mi_orders` routes this order to the fused kernels
        (measured, profiles/mi.txt)."""
        from . import backend
        return _hip.mi_covered(moving, fixed, disp, weight, order, bins) and int(order[0]) in backend.fused_mi_orders

    @staticmethod
    def mi_gauss_newton(moving, fixed, disp, weight, ranges, bound, order, extrapolate, hessian, bins, return_histogram):
        """(loss, gradient, hessian | None, histogram | None): the fused kernels (csrc/mi.hip) where they apply, else the composed
        form."""
        if _HipKernels.mi_fused(moving, fixed, disp, weight, order, bins):
            return _hip.mi(moving, fixed, disp, weight, ranges, bound, order, extrapolate, hessian, bins, return_histogram)
        from .torch_kernels import mi_gauss_newton_composed
        return mi_gauss_newton_composed(moving, fixed, disp, weight, ranges, bound, order, extrapolate, hessian, bins, return_histogram)

    @staticmethod
    def spline_filter_(data, bound, order, dim, src=None):
        return _hip.spline_filter_(data, bound, order, dim, src=src)

    @staticmethod
    def pull_labels(inp, grid, bound, order, extrapolate, displacement=False):
        return _hip.pull_labels(inp, grid, bound, order, extrapolate, flags=_dflag(displacement))

    @staticmethod
    def resample1d(src, lin, dim, order, bound, extrapolate, mode, adjoint, n_lattice):
        return _hip.resample1d(src, lin, dim, order, bound, extrapolate, mode, adjoint, n_lattice)


_kernels = _HipKernels


@contextlib.contextmanager
def use_kernels(table):
    """TEST HOOK: temporarily replace the kernel table (see module docstring)."""
    global _kernels
    old = _kernels
    _kernels = table
    try:
        yield
    finally:
        _kernels = old


def kernels(*tensors, dim=None):
    """The kernel table that serves these tensors: the HIP library for CUDA tensors of 1-3 spatial dims (it raises when
    libinterpol_hip.so is missing: there is no silent fallback on the GPU), the device-generic PyTorch restatement
    (interpol/torch_kernels.py) for what the library does not cover -- CPU tensors and D > 3, which the reference's nd
    path accepts (pushpull.py:49-66).  A table installed with `use_kernels` (tests) always wins."""
    if _kernels is not _HipKernels:
        return _kernels
    on_gpu = True
    for t in tensors:
        dev = getattr(t, 'device', None)
        if dev is not None and torch.device(dev).type != 'cuda':
            on_gpu = False
    if on_gpu and (dim is None or dim <= 3):
        return _HipKernels
    from .torch_kernels import TorchKernels
    return TorchKernels


def _codes(grid, bound, interpolation):
    dim = grid.shape[-1]
    return pad_codes(bound, dim), pad_codes(interpolation, dim)


def _check_push_shapes(inp, grid, trailing=0):
    dim = grid.shape[-1]
    isp = tuple(inp.shape[2:2 + dim]) if trailing else tuple(inp.shape[-dim:])
    if isp != tuple(grid.shape[1:-1]):
        # reference interpol/iso1.py:149-150, iso0.py:82-83
        raise ValueError('Input and grid should have the same spatial shape')


def grid_pull(inp, grid, bound, interpolation, extrapolate, displacement=False):
    """(B,C,*in), (B,*out,D) -> (B,C,*out).   Reference pushpull.py:35-66."""
    bound, interpolation = _codes(grid, bound, interpolation)
    return kernels(inp, grid, dim=grid.shape[-1]).pull(inp, grid, bound, interpolation, int(extrapolate), **_kw(displacement))


def grid_push(inp, grid, shape, bound, interpolation, extrapolate, displacement=False):
    """(B,C,*in), (B,*in,D) -> (B,C,*shape).   Reference pushpull.py:70-102."""
    bound, interpolation = _codes(grid, bound, interpolation)
    _check_push_shapes(inp, grid)
    shape = None if shape is None else list(shape)
    return kernels(inp, grid, dim=grid.shape[-1]).push(inp, grid, shape, bound, interpolation, int(extrapolate), **_kw(displacement))


def grid_count(grid, shape, bound, interpolation, extrapolate, displacement=False):
    """(B,*in,D) -> (B,1,*shape).   Reference pushpull.py:106-142."""
    bound, interpolation = _codes(grid, bound, interpolation)
    shape = None if shape is None else list(shape)
    return kernels(grid, dim=grid.shape[-1]).count(grid, shape, bound, interpolation, int(extrapolate), **_kw(displacement))


def grid_grad(inp, grid, bound, interpolation, extrapolate, displacement=False):
    """(B,C,*in), (B,*out,D) -> (B,C,*out,D).   Reference pushpull.py:146-172."""
    bound, interpolation = _codes(grid, bound, interpolation)
    return kernels(inp, grid, dim=grid.shape[-1]).grad(inp, grid, bound, interpolation, int(extrapolate), **_kw(displacement))


def grid_pushgrad(inp, grid, shape, bound, interpolation, extrapolate, displacement=False):
    """(B,C,*in,D), (B,*in,D) -> (B,C,*shape).   Reference pushpull.py:176-203."""
    bound, interpolation = _codes(grid, bound, interpolation)
    _check_push_shapes(inp, grid, trailing=1)
    shape = None if shape is None else list(shape)
    return kernels(inp, grid, dim=grid.shape[-1]).pushgrad(inp, grid, shape, bound, interpolation, int(extrapolate), **_kw(displacement))


def grid_hess(inp, grid, bound, interpolation, extrapolate, displacement=False):
    """(B,C,*in), (B,*out,D) -> (B,C,*out,D,D).   Reference pushpull.py:207-233."""
    bound, interpolation = _codes(grid, bound, interpolation)
    return kernels(inp, grid, dim=grid.shape[-1]).hess(inp, grid, bound, interpolation, int(extrapolate), **_kw(displacement))


def grid_pull_backward(grad, inp, grid, bound, interpolation, extrapolate,
                       need_inp=None, need_grid=None, displacement=False):
    """-> (grad_inp (B,C,*in) | None, grad_grid (B,*out,D) | None).
    Reference pushpull.py:237-258; gradients are only computed for the inputs
    that require them (pushpull.py:252-255)."""
    bound, interpolation = _codes(grid, bound, interpolation)
    need_inp = inp.requires_grad if need_inp is None else need_inp
    need_grid = grid.requires_grad if need_grid is None else need_grid
    if not (need_inp or need_grid):
        return None, None
    return kernels(grad, inp, grid, dim=grid.shape[-1]).pull_backward(grad, inp, grid, bound, interpolation, int(extrapolate), need_inp, need_grid,
                                  **_kw(displacement))


def grid_push_backward(grad, inp, grid, bound, interpolation, extrapolate,
                       need_inp=None, need_grid=None, displacement=False):
    """-> (grad_inp (B,C,*in) | None, grad_grid (B,*in,D) | None).
    Reference pushpull.py:262-282."""
    bound, interpolation = _codes(grid, bound, interpolation)
    need_inp = inp.requires_grad if need_inp is None else need_inp
    need_grid = grid.requires_grad if need_grid is None else need_grid
    if not (need_inp or need_grid):
        return None, None
    return kernels(grad, inp, grid, dim=grid.shape[-1]).push_backward(grad, inp, grid, bound, interpolation, int(extrapolate), need_inp, need_grid,
                                  **_kw(displacement))


def grid_count_backward(grad, grid, bound, interpolation, extrapolate, need_grid=None, displacement=False):
    """-> grad_grid (B,*in,D) | None.   Reference pushpull.py:286-299."""
    bound, interpolation = _codes(grid, bound, interpolation)
    need_grid = grid.requires_grad if need_grid is None else need_grid
    if not need_grid:
        return None
    return kernels(grad, grid, dim=grid.shape[-1]).count_backward(grad, grid, bound, interpolation, int(extrapolate), **_kw(displacement))


def grid_pull_backward_affine(grad, inp, lattice, bound, interpolation, extrapolate):
    """Gradient of grid_pull(inp, AffineGrid(mat, shape)) with respect to `mat`: grad (B,C,*shape), inp (B,C,*in) -> (D, D+1),
    summed over the batch.  The chain rule of pushpull.py:237-258 through affine_grid (api.py:534-572); on the GPU the
    (B,*shape,D) grid gradient is reduced against the sample index inside the kernel (csrc/affine_grad.hip)."""
    bound, interpolation = _codes(lattice, bound, interpolation)
    return kernels(grad, inp, lattice, dim=lattice.shape[-1]).affine_pull_backward(grad, inp, lattice, bound, interpolation, int(extrapolate))


def grid_push_backward_affine(grad, inp, lattice, bound, interpolation, extrapolate):
    """Gradient of grid_push(inp, AffineGrid(mat, inshape), shape) -- inp None: of grid_count -- with respect to `mat`:
    grad (B,C,*shape), inp (B,C,*inshape) -> (D, D+1), summed over the batch.  pushpull.py:262-299 through affine_grid."""
    bound, interpolation = _codes(lattice, bound, interpolation)
    return kernels(grad, inp, lattice, dim=lattice.shape[-1]).affine_push_backward(grad, inp, lattice, bound, interpolation, int(extrapolate))


def grid_grad_backward(grad, inp, grid, bound, interpolation, extrapolate,
                       need_inp=None, need_grid=None, displacement=False):
    """-> (grad_inp (B,C,*in) | None, grad_grid (B,*out,D) | None); only reached
    by double backward.   Reference pushpull.py:303-325."""
    dim = grid.shape[-1]
    need_inp = inp.requires_grad if need_inp is None else need_inp
    need_grid = grid.requires_grad if need_grid is None else need_grid
    grad_inp = grad_grid = None
    if need_inp:
        grad_inp = grid_pushgrad(grad, grid, inp.shape[-dim:], bound, interpolation, extrapolate, displacement)
    if need_grid:
        hess = grid_hess(inp, grid, bound, interpolation, extrapolate, displacement)
        grad_grid = (hess * grad.unsqueeze(-1)).sum(dim=[1, -2])
    return grad_inp, grad_grid


def resample1d(src, lin, dim, order, bound, extrapolate, mode, adjoint=False, n_lattice=None):
    """One 1-D pass of a tensor-product resampling along `dim` (see `separable.py`):
    forward = pull along that dim at coordinates `lin`, adjoint = the matching push."""
    return kernels(src, lin).resample1d(src, lin, dim, int(order), int(bound), int(extrapolate), int(mode), bool(adjoint), n_lattice)


def labels_covered(dim, interpolation, *tensors):
    """Can `grid_pull_labels` serve this stencil (else the caller loops over the labels)?"""
    if dim > 3 or kernels(*tensors, dim=dim) is not _HipKernels:
        return False
    return _hip.labels_covered(dim, pad_codes(interpolation, dim))


def grid_pull_labels(inp, grid, bound, interpolation, extrapolate, displacement=False):
    """Integer label map (B,C,*in), float32 grid (B,*out,D) -> int32 (B,C,*out): the label whose
    interpolated indicator image is largest (> 0), smallest label on ties, else 0 -- the result of
    the reference's loop over `input.unique()` (api.py:194-205, prefilter=False) in one pass."""
    bound, interpolation = _codes(grid, bound, interpolation)
    return kernels(inp, grid, dim=grid.shape[-1]).pull_labels(inp, grid, bound, interpolation, int(extrapolate), **_kw(displacement))


def compose_covered(left, right, orders):
    """Does the fused kernel (csrc/compose.hip) serve `compose(left, right)` -- else it is composed from grid_pull?
    GPU fields of one float32 / float64 dtype, D <= 3, one order for all dims that the library instantiates (1..3) and that
    `backend.fused_compose_orders` routes there (the orders at which the fused kernel was measured faster)."""
    dim = right.shape[-1]
    if dim > 3 or kernels(left, right, dim=dim) is not _HipKernels:
        return False
    return _HipKernels.compose_fused(left, right, pad_codes(orders, dim))


def compose(left, right, bound, interpolation, extrapolate, out=None):
    """Displacement fields (B|1,*lshape,D), (B|1,*oshape,D) -> right + pull(left, id + right), (B,*oshape,D): what
    `right + grid_pull(left.movedim(-1, 1), right, ..., displacement=True).movedim(1, -1)` computes.
    `out`: a dense (B,*oshape,D) tensor to write into; it may be `right` itself, it must not share memory with `left`."""
    bound, interpolation = _codes(right, bound, interpolation)
    return kernels(left, right, dim=right.shape[-1]).compose(left, right, bound, interpolation, int(extrapolate), out=out)


def compose_backward(grad, left, right, bound, interpolation, extrapolate, need_left=None, need_right=None):
    """-> (grad_left (B,*lshape,D) | None, grad_right (B,*oshape,D) | None), one per batch item of `grad`."""
    bound, interpolation = _codes(right, bound, interpolation)
    need_left = left.requires_grad if need_left is None else need_left
    need_right = right.requires_grad if need_right is None else need_right
    if not (need_left or need_right):
        return None, None
    return kernels(grad, left, right, dim=right.shape[-1]).compose_backward(grad, left, right, bound, interpolation, int(extrapolate),
                                                                           need_left, need_right)


def jacobian_covered(disp, orders):
    """Do the fused kernels (csrc/jacobian.hip) serve `jacobian(disp)` / `jacdet(disp)` -- else they are composed from grid_grad?
    A GPU field (B,*shape,D) of dtype float32 / float64, D <= 3, one order for all dims that the library instantiates (1..3) and
    that `backend.fused_jacobian_orders` routes there."""
    dim = disp.shape[-1]
    if dim > 3 or kernels(disp, dim=dim) is not _HipKernels:
        return False
    return _HipKernels.jacobian_fused(disp, pad_codes(orders, dim))


def jacobian(disp, bound, interpolation, add_identity=True):
    """Displacement field (B,*shape,D) -> (B,*shape,D,D): what `grid_grad(disp.movedim(-1, 1), zeros, ..., extrapolate=True,
    displacement=True).movedim(1, -2) + eye(D)` computes (row = component, column = direction)."""
    bound, interpolation = _codes(disp, bound, interpolation)
    return kernels(disp, dim=disp.shape[-1]).jacobian(disp, bound, interpolation, bool(add_identity))


def jacdet(disp, bound, interpolation):
    """Displacement field (B,*shape,D) -> det(jacobian(disp)), (B,*shape)."""
    bound, interpolation = _codes(disp, bound, interpolation)
    return kernels(disp, dim=disp.shape[-1]).jacdet(disp, bound, interpolation)


def jacobian_backward(grad, bound, interpolation):
    """grad (B,*shape,D,D) -> the gradient of `jacobian` with respect to the field, (B,*shape,D)."""
    dim = grad.shape[-1]
    return kernels(grad, dim=dim).jacobian_backward(grad, pad_codes(bound, dim), pad_codes(interpolation, dim))


def jacdet_backward(grad, disp, bound, interpolation):
    """grad (B,*shape) -> the gradient of `jacdet` with respect to the field, (B,*shape,D)."""
    bound, interpolation = _codes(disp, bound, interpolation)
    return kernels(grad, disp, dim=disp.shape[-1]).jacdet_backward(grad, disp, bound, interpolation)


def regulariser_covered(field):
    """Do the fused kernels (csrc/regulariser.hip) serve `regulariser(field)` / `regulariser_energy(field)` -- else the composed
    form does?  A GPU field (B,*shape,D) of dtype float32 / float64, D <= 3, while `backend.fused_regulariser` is set."""
    dim = field.shape[-1]
    if dim > 3 or kernels(field, dim=dim) is not _HipKernels:
        return False
    return _HipKernels.regulariser_fused(field)


def regulariser(field, weights, voxel_size, bound):
    """Displacement field (B,*shape,D) -> L field, (B,*shape,D).  weights = (absolute, membrane, bending) or
    (absolute, membrane, bending, shears, div): non-negative floats, not all zero; voxel_size: D positive floats; bound: codes
    (0..6, and 7 = sliding), padded to D."""
    dim = field.shape[-1]
    return kernels(field, dim=dim).regulariser(field, tuple(weights), list(voxel_size), pad_codes(bound, dim))


def regulariser_energy(field, weights, voxel_size, bound):
    """Displacement field (B,*shape,D) -> 0.5 <field, L field> per batch item, (B)."""
    dim = field.shape[-1]
    return kernels(field, dim=dim).regulariser_energy(field, tuple(weights), list(voxel_size), pad_codes(bound, dim))


def regulariser_solve_covered(gradient, hessian=None):
    """Do the fused kernels (csrc/regulariser_solve.hip) serve `regulariser_solve(gradient, hessian)` -- else the composed form
    does?  GPU tensors (B,*shape,D) / (B|1,*shape,K) of dtype float32 / float64, D <= 3, while `backend.fused_regulariser_solve`
    is set."""
    dim = gradient.shape[-1]
    if dim > 3 or kernels(gradient, hessian, dim=dim) is not _HipKernels:
        return False
    return _HipKernels.regulariser_solve_fused(gradient, hessian)


def regulariser_solve(gradient, hessian, weights, voxel_size, bound, max_iter, tolerance):
    """gradient (B,*shape,D), hessian None or (B|1,*shape,K) -> (x, iterations, residual): x (B,*shape,D) after at most `max_iter`
    preconditioned conjugate-gradient iterations on (H + L) x = gradient, iterations (B) int64, residual (B) float64.  weights,
    voxel_size, bound as for `regulariser`, the bounds out of zero, dft, sliding and -- without shears and div -- dct2, dst2.
    Nothing synchronises."""
    dim = gradient.shape[-1]
    return kernels(gradient, hessian, dim=dim).regulariser_solve(gradient, hessian, tuple(weights), list(voxel_size),
                                                                 pad_codes(bound, dim), int(max_iter), float(tolerance))


def regulariser_multigrid_covered(gradient, hessian=None):
    """Do the fused kernels (csrc/regulariser_multigrid.hip) serve `regulariser_solve(..., preconditioner='multigrid')` -- else the
    composed form does?  As `regulariser_solve_covered`, while `backend.fused_regulariser_multigrid` is set."""
    dim = gradient.shape[-1]
    if dim > 3 or kernels(gradient, hessian, dim=dim) is not _HipKernels:
        return False
    return _HipKernels.regulariser_multigrid_fused(gradient, hessian)


def regulariser_multigrid(gradient, hessian, weights, voxel_size, bound, max_iter, tolerance, smoothing):
    """`regulariser_solve` with one multigrid V-cycle (`smoothing` sweeps before and after the coarse correction) as the
    preconditioner of the conjugate gradients -> (x, iterations, residual).  Nothing synchronises."""
    dim = gradient.shape[-1]
    return kernels(gradient, hessian, dim=dim).regulariser_multigrid(gradient, hessian, tuple(weights), list(voxel_size),
                                                                     pad_codes(bound, dim), int(max_iter), float(tolerance), int(smoothing))


def regulariser_vcycle(residual, hessian, weights, voxel_size, bound, smoothing=2):
    """z = V(residual): one V-cycle of the multigrid preconditioner alone, (B,*shape,D) (tests and timing; not part of the public
    namespace)."""
    dim = residual.shape[-1]
    return kernels(residual, hessian, dim=dim).regulariser_vcycle(residual, hessian, tuple(weights), list(voxel_size),
                                                                  pad_codes(bound, dim), int(smoothing))


def ssd_covered(moving, fixed, disp, weight, orders, hessian='full'):
    """Does the fused kernel (csrc/ssd.hip) serve `ssd_gauss_newton(moving, fixed, disp, weight, hessian=hessian)` -- else the
    composed form does?  GPU tensors of one float32 / float64 dtype, D <= 3, one order for all dims that the library instantiates
    (1..3) and that `backend.fused_ssd_orders` (without a Hessian: `backend.fused_ssd_orders_without_hessian` as well) routes there."""
    dim = disp.shape[-1]
    if dim > 3 or kernels(moving, fixed, disp, weight, dim=dim) is not _HipKernels:
        return False
    return _HipKernels.ssd_fused(moving, fixed, disp, weight, pad_codes(orders, dim), hessian)


def ssd_gauss_newton(moving, fixed, disp, weight, bound, interpolation, extrapolate, hessian):
    """moving (B|1,C,*inshape), fixed (B|1,C,*shape), disp (B|1,*shape,D), weight None or (B|1,*shape) -> (loss (B), gradient
    (B,*shape,D), hessian (B,*shape,K) | None) of 0.5 sum weight (moving(id + disp) - fixed)^2 with respect to `disp`.
    hessian: None, 'diagonal' (K = D) or 'full' (K = D (D + 1) / 2).  Nothing synchronises."""
    bound, interpolation = _codes(disp, bound, interpolation)
    return kernels(moving, fixed, disp, weight, dim=disp.shape[-1]).ssd_gauss_newton(moving, fixed, disp, weight, bound, interpolation,
                                                                                    int(extrapolate), hessian)


def lcc_covered(moving, fixed, disp, weight, orders, window):
    """Do the fused kernels (csrc/lcc.hip) serve `lcc_gauss_newton(moving, fixed, disp, weight, window=window)` -- else the composed
    form does?  GPU tensors of one float32 / float64 dtype, D <= 3, odd windows up to 9, one order for all dims that the library
    instantiates (1..3) and that `backend.fused_lcc_orders` routes there."""
    dim = disp.shape[-1]
    if dim > 3 or kernels(moving, fixed, disp, weight, dim=dim) is not _HipKernels:
        return False
    return _HipKernels.lcc_fused(moving, fixed, disp, weight, pad_codes(orders, dim), pad_codes(list(window), dim))


def lcc_gauss_newton(moving, fixed, disp, weight, bound, interpolation, extrapolate, hessian, window, eps):
    """moving (B|1,C,*inshape), fixed (B|1,C,*shape), disp (B|1,*shape,D), weight None or (B|1,*shape) -> (loss (B), gradient
    (B,*shape,D), hessian (B,*shape,K) | None) of the local normalised cross-correlation over `window` (D odd ints) with respect
    to `disp`.  hessian: None, 'diagonal' (K = D) or 'full' (K = D (D + 1) / 2).  Nothing synchronises."""
    bound, interpolation = _codes(disp, bound, interpolation)
    return kernels(moving, fixed, disp, weight, dim=disp.shape[-1]).lcc_gauss_newton(moving, fixed, disp, weight, bound, interpolation,
                                                                                    int(extrapolate), hessian, [int(w) for w in window],
                                                                                    float(eps))


def ssd_affine_covered(moving, fixed, mat, weight, orders):
    """Does the fused kernel (csrc/ssd_affine.hip) serve `ssd_gauss_newton_affine(moving, fixed, mat, weight)` -- else the composed
    form does?  GPU tensors of one float32 / float64 dtype, D <= 3, one order for all dims that the library instantiates (1..3) and
    that `backend.fused_ssd_affine_orders` routes there."""
    dim = mat.shape[-1] - 1
    if dim > 3 or kernels(moving, fixed, mat, weight, dim=dim) is not _HipKernels:
        return False
    return _HipKernels.ssd_affine_fused(moving, fixed, mat, weight, pad_codes(orders, dim))


def ssd_gauss_newton_affine(moving, fixed, mat, weight, bound, interpolation, extrapolate, hessian):
    """moving (B|1,C,*inshape), fixed (B|1,C,*shape), mat (B|1,D,D+1), weight None or (B|1,*shape) -> (loss (B), gradient (B,D,D+1),
    hessian (B,P,P) | None, P = D (D+1)) of 0.5 sum weight (moving(A o + t) - fixed)^2 with respect to the matrix of each item.
    Nothing synchronises."""
    dim = mat.shape[-1] - 1
    bound, interpolation = pad_codes(bound, dim), pad_codes(interpolation, dim)
    return kernels(moving, fixed, mat, weight, dim=dim).ssd_gauss_newton_affine(moving, fixed, mat, weight, bound, interpolation,
                                                                                 int(extrapolate), bool(hessian))


def lcc_affine_covered(moving, fixed, mat, weight, orders, window):
    """Do the fused kernels (csrc/lcc_affine.hip) serve `lcc_gauss_newton_affine(moving, fixed, mat, weight, window=window)` -- else
    the composed form does?  GPU tensors of one float32 / float64 dtype, D <= 3, odd windows up to 9, one order for all dims that the
    library instantiates (1..3) and that `backend.fused_lcc_affine_orders` routes there."""
    dim = mat.shape[-1] - 1
    if dim > 3 or kernels(moving, fixed, mat, weight, dim=dim) is not _HipKernels:
        return False
    return _HipKernels.lcc_affine_fused(moving, fixed, mat, weight, pad_codes(orders, dim), pad_codes(list(window), dim))


def lcc_gauss_newton_affine(moving, fixed, mat, weight, bound, interpolation, extrapolate, hessian, window, eps):
    """moving (B|1,C,*inshape), fixed (B|1,C,*shape), mat (B|1,D,D+1), weight None or (B|1,*shape) -> (loss (B), gradient (B,D,D+1),
    hessian (B,P,P) | None, P = D (D+1)) of the local normalised cross-correlation over `window` (D odd ints) between moving(A o + t)
    and fixed with respect to the matrix of each item.  Nothing synchronises."""
    dim = mat.shape[-1] - 1
    bound, interpolation = pad_codes(bound, dim), pad_codes(interpolation, dim)
    return kernels(moving, fixed, mat, weight, dim=dim).lcc_gauss_newton_affine(moving, fixed, mat, weight, bound, interpolation,
                                                                                 int(extrapolate), bool(hessian),
                                                                                 [int(w) for w in window], float(eps))


def mi_affine_covered(moving, fixed, mat, weight, orders, bins=32):
    """Do the fused kernels (csrc/mi_affine.hip) serve `mi_gauss_newton_affine(moving, fixed, mat, weight, bins=bins)` -- else the
    composed form does?  GPU tensors of one float32 / float64 dtype, D <= 3, one channel, 8 <= bins <= 64, one order for all dims that
    the library instantiates (1..3) and that `backend.fused_mi_affine_orders` routes there."""
    dim = mat.shape[-1] - 1
    if dim > 3 or kernels(moving, fixed, mat, weight, dim=dim) is not _HipKernels:
        return False
    return _HipKernels.mi_affine_fused(moving, fixed, mat, weight, pad_codes(orders, dim), bins)


def mi_gauss_newton_affine(moving, fixed, mat, weight, bound, interpolation, extrapolate, hessian, bins=32, moving_range=None,
                           fixed_range=None, return_histogram=False):
    """moving (B|1,1,*inshape), fixed (B|1,1,*shape), mat (B|1,D,D+1), weight None or (B|1,*shape) -> (loss (B), gradient (B,D,D+1),
    hessian (B,P,P) | None, histogram (B,bins,bins) | None) of minus the mutual information with respect to the matrix of each item.
    The ranges ((lo, hi) or None = aminmax per item) are formed on the device (`torch_kernels.mi_ranges`).  Nothing synchronises."""
    from .torch_kernels import mi_ranges
    dim = mat.shape[-1] - 1
    bound, interpolation = pad_codes(bound, dim), pad_codes(interpolation, dim)
    B = max(moving.shape[0], fixed.shape[0], mat.shape[0], 1 if weight is None else weight.shape[0])
    ranges = mi_ranges(moving, fixed, weight, moving_range, fixed_range, B)
    return kernels(moving, fixed, mat, weight, dim=dim).mi_gauss_newton_affine(moving, fixed, mat, weight, ranges, bound, interpolation,
                                                                                int(extrapolate), bool(hessian), int(bins),
                                                                                bool(return_histogram))


def mi_covered(moving, fixed, disp, weight, orders, bins=32):
    """Do the fused kernels (csrc/mi.hip) serve `mi_gauss_newton(moving, fixed, disp, weight, bins=bins)` -- else the composed form
    does?  GPU tensors of one float32 / float64 dtype, D <= 3, one channel, 8 <= bins <= 64, one order for all dims that the library
    instantiates (1..3) and that `backend.fused_mi_orders` routes there."""
    dim = disp.shape[-1]
    if dim > 3 or kernels(moving, fixed, disp, weight, dim=dim) is not _HipKernels:
        return False
    return _HipKernels.mi_fused(moving, fixed, disp, weight, pad_codes(orders, dim), bins)


def mi_gauss_newton(moving, fixed, disp, weight, bound, interpolation, extrapolate, hessian, bins=32, moving_range=None,
                    fixed_range=None, return_histogram=False):
    """moving (B|1,1,*inshape), fixed (B|1,1,*shape), disp (B|1,*shape,D), weight None or (B|1,*shape) -> (loss (B), gradient
    (B,*shape,D), hessian (B,*shape,K) | None, histogram (B,bins,bins) | None) of minus the mutual information with respect to `disp`.
    hessian: None, 'diagonal' (K = D) or 'full' (K = D (D + 1) / 2).  The ranges ((lo, hi) or None = aminmax per item) are formed on
    the device (`torch_kernels.mi_ranges`).  Nothing synchronises."""
    from .torch_kernels import mi_ranges
    bound, interpolation = _codes(disp, bound, interpolation)
    B = max(moving.shape[0], fixed.shape[0], disp.shape[0], 1 if weight is None else weight.shape[0])
    ranges = mi_ranges(moving, fixed, weight, moving_range, fixed_range, B)
    return kernels(moving, fixed, disp, weight, dim=disp.shape[-1]).mi_gauss_newton(moving, fixed, disp, weight, ranges, bound,
                                                                                   interpolation, int(extrapolate), hessian, int(bins),
                                                                                   bool(return_histogram))


def grid_push_count(inp, grid, shape, bound, interpolation, extrapolate, displacement=False):
    """(B,C,*in), (B,*in,D) -> (B,C+1,*shape): grid_push of `inp` in channels 0..C-1 and grid_count
    of the same grid in channel C, from ONE pass over the grid (pushpull.py:70-102 + 106-142)."""
    bound, interpolation = _codes(grid, bound, interpolation)
    _check_push_shapes(inp, grid)
    shape = None if shape is None else list(shape)
    return kernels(inp, grid, dim=grid.shape[-1]).push_count(inp, grid, shape, bound, interpolation, int(extrapolate), **_kw(displacement))
