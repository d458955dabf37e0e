"""The second-order operators -- grid_hess, grid_pushgrad and the grid_grad_backward composed of them -- under a mask.

The reference raises for `nd.hess` with extrapolate in {0, 2} (SURVEY B-2), so no stored or live result of it can pin the masked
Hessian.  What pins it is an identity: the mask of nd.py:10-27 multiplies the result, so for ex in {0, 2}

    hess_ex(inp, grid)     = hess_1(inp, grid) * inside_ex(grid)[:, None, ..., None, None]
    pushgrad_ex(val, grid) = pushgrad_1(val * inside_ex(grid)[:, None, ..., None], grid)
    inside_ex: every coordinate strictly between -thr and n_d - 1 + thr, thr = 0.05 (ex = 0) / 0.55 (ex = 2)

and the extrapolate = 1 results of the oracle are pinned against the reference for every order and bound, float32 and float64
(tests/test_oracle_vs_reference.py).  `masked_truth` below is that identity in numpy float64 and the ONLY source of a masked expected
value, here and in tests/test_second_order_gpu.py (which imports the inputs, the shapes and the bars from this module).

Inputs (`problem`).  Coordinates are multiples of 1/64 of magnitude < 128 (tests/test_compose_gpu.py uses the same device): exact
in float32 and float64 alike, so both see the same `floor` and the same mask, and no mask threshold (a multiple of 0.05 that is
no multiple of 1/64) lies on one; many samples fall exactly on knots and half-knots.  The grid is an identity scaled to overhang
the lattice by OVERHANG[dim] voxels on each side plus uniform dyadic noise of +-1 voxel.  The overhang is 5 / 2 / 0.75 voxels in
1 / 2 / 3 dimensions: the share of samples outside the field of view grows with every dimension (the noise carries samples near
a face across it), and 2 voxels would mask 6 % of the 67-point line and two thirds of (13, 10, 17); with these it is 13.5 %,
44 % and 47 % at ex = 0.  `problem` itself asserts, for shapes whose every
extent is >= 10, that ex = 0 masks between 10 % and 60 % of the samples and ex = 2 strictly fewer, but some.  The values (inp, val,
grad) are independent randn in every component, rounded to float32 so that one float64 truth serves both precisions; B = 2, C = 3.

Bars (`ratio`): |got - want| <= tol |want| + tol scale, scale = max(max|want|, max|input values|).  The floor by the input is
needed where the derivative is identically zero (a 1-point lattice with a replicating bound): the oracle returns rounding noise
of 1e-17 there and a bar relative to it is meaningless; B-spline derivative weights are O(1) in voxel units, so an error below
tol max|input| is below what cancellation in that precision delivers.  tol: 1e-12 on the CPU (float64 against float64).
"""
import os

import numpy as np
import pytest
import torch

from interpol.torch_kernels import TorchKernels
from oracle import oracle

B, C = 2, 3
OVERHANG = {1: 5.0, 2: 2.0, 3: 0.75}
# (lattice, samples) per dim: the first has every extent >= 10, the others are 1 - 4 point lattices that an order-7 stencil wraps
# several times (dst1's zero sign at index 0 included)
SHAPES = {1: [((67,), (300,)), ((1,), (40,)), ((2,), (40,))],
          2: [((13, 22), (19, 11)), ((1, 4), (5, 8))],
          3: [((13, 10, 17), (11, 14, 9)), ((2, 1, 3), (5, 4, 3))]}
# what the CPU sweeps of the PyTorch table run on (it is a Python loop over (K+1)^D taps): the tiny lattices above and these
SMALL = {1: ((9,), (40,)), 2: ((5, 6), (7, 6)), 3: ((5, 6, 7), (6, 4, 5))}
# tests/golden/make_golden.py: mixed()
MIXED = [([2, 3, 5], [2, 5, 0]), ([1, 3], [6, 1, 3]), ([0, 3], [3]), ([3, 1, 2], [4, 2, 6]),
         ([2, 3], [2, 5]), ([7, 0, 4], [1]), ([1, 1, 0], [0, 4, 5]), ([3, 3, 3, 1], [3, 3, 3, 0])]
THRESHOLD = {0: 0.05, 2: 0.55}
_PROBLEMS = {}


def inside(grid, lattice, ex):
    """nd.py:10-27 in numpy float64: bool (B, *samples), all True for ex = 1"""
    g = np.asarray(grid, dtype=np.float64)
    m = np.ones(g.shape[:-1], dtype=bool)
    if ex == 1:
        return m
    thr = THRESHOLD[ex]
    for d, n in enumerate(lattice):
        m &= (g[..., d] > -thr) & (g[..., d] < n - 1 + thr)
    return m


def _np(t):
    return t.detach().cpu().double().numpy() if torch.is_tensor(t) else np.asarray(t, dtype=np.float64)


def masked_truth(op, a, grid, bound, order, ex, shape=None, grad=None, base=None):
    """The identity of the module docstring from the oracle at extrapolate = 1, numpy float64.
      "hess":          a = inp (B,C,*lattice)                       -> (B,C,*samples,D,D)
      "pushgrad":      a = val (B,C,*samples,D), shape = lattice    -> (B,C,*lattice)
      "grad_backward": a = inp, grad = (B,C,*samples,D)             -> (grad_inp, grad_grid), pushpull.py:303-325
    `base`: the oracle's extrapolate = 1 Hessian of the same call, where the caller has it already."""
    a, grid = _np(a), _np(grid)
    dim = grid.shape[-1]
    if op == "hess":
        m = inside(grid, a.shape[-dim:], ex)
        h = np.asarray(oracle.grid_hess(a, grid, bound, order, 1)) if base is None else base
        return h * m[(slice(None), None) + (Ellipsis, None, None)]
    if op == "pushgrad":
        m = inside(grid, shape, ex)
        return np.asarray(oracle.grid_pushgrad(a * m[:, None, ..., None], grid, list(shape), bound, order, 1))
    if op == "grad_backward":
        g = _np(grad)
        gi = masked_truth("pushgrad", g, grid, bound, order, ex, shape=a.shape[-dim:])
        hh = masked_truth("hess", a, grid, bound, order, ex, base=base)
        return gi, (hh * g[..., None]).sum(axis=(1, -2))
    raise ValueError(op)


def masked_share(grid, lattice, ex):
    return 1.0 - float(inside(grid, lattice, ex).mean())


def dyadic_line(n, m, h, dtype=torch.float64):
    """m coordinates from -h to n - 1 + h, rounded to multiples of 1/64"""
    return torch.round(torch.linspace(-h, n - 1 + h, m, dtype=torch.float64) * 64).div(64).to(dtype)


def problem(lattice, samples, seed=0):
    """-> dict(inp (B,C,*lattice), val, grad (B,C,*samples,D), grid (B,*samples,D)): float64 CPU tensors of float32-representable
    values, built once per (lattice, samples, seed) and never modified."""
    key = (tuple(lattice), tuple(samples), seed)
    if key in _PROBLEMS:
        return _PROBLEMS[key]
    dim = len(lattice)
    gen = torch.Generator().manual_seed(1000 * dim + 17 * sum(lattice) + seed)
    h = OVERHANG[dim]
    lins = [dyadic_line(n, m, h) for n, m in zip(lattice, samples)]
    grid = torch.stack(torch.meshgrid(*lins, indexing="ij"), -1)[None]
    grid = grid + torch.randint(-64, 65, [B, *samples, dim], generator=gen).double() / 64
    assert float(grid.abs().max()) < 128 and torch.equal(grid * 64, torch.round(grid * 64)) and torch.equal(grid.float().double(), grid)
    r = lambda *s: torch.randn(*s, generator=gen).double()           # (float32 randn: representable in both precisions)
    p = dict(inp=r(B, C, *lattice), val=r(B, C, *samples, dim), grad=r(B, C, *samples, dim), grid=grid.contiguous(),
             lattice=list(lattice), samples=list(samples))
    if min(lattice) >= 10:
        s0, s2 = masked_share(grid, lattice, 0), masked_share(grid, lattice, 2)
        assert 0.10 <= s0 <= 0.60, (key, s0)
        assert 0.0 < s2 < s0, (key, s2, s0)
    _PROBLEMS[key] = p
    return p


def ratio(got, want, tol, floor):
    """worst |got - want| / (tol |want| + tol max(max|want|, floor)); got must be finite"""
    got, want = _np(got), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if want.size == 0:
        return 0.0
    assert np.isfinite(got).all()
    scale = max(float(np.abs(want).max()), float(floor))
    return float((np.abs(got - want) / (tol * np.abs(want) + tol * scale)).max())


def amax(*ts):
    return max(float(np.abs(_np(t)).max()) for t in ts)


def stencils(dim):
    """every order x every bound, one for all dims, and the mixed combinations of make_golden.mixed()"""
    return [([k], [b]) for k in range(8) for b in range(7)] + [(o, b) for o, b in MIXED]


def test_mixed_combinations_are_those_of_the_golden_generator():
    import ast
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_golden.py")).read()
    at = src.index("combos = [", src.index("def mixed():"))
    end = src.index("\n    for dim", at)
    assert ast.literal_eval(src[at + len("combos = "):end].strip()) == MIXED


def test_committed_seeds_mask_the_stated_share():
    """(problem() asserts it; this states the figures where a reader finds them)"""
    for dim in (1, 2, 3):
        lattice, samples = SHAPES[dim][0]
        g = problem(lattice, samples)["grid"]
        s0, s2 = masked_share(g, lattice, 0), masked_share(g, lattice, 2)
        print("masked share %s <- %s: ex=0 %.3f, ex=2 %.3f" % (lattice, samples, s0, s2))
        assert 0.10 <= s0 <= 0.60 and 0.0 < s2 < s0
        on_knot = float((g == torch.round(g)).float().mean())
        assert on_knot > 0.005                                  # (samples exactly on knots are wanted)


def _run(dim, shapes, hess, pushgrad, grad_backward, tol, what):
    worst = 0.0
    for lattice, samples in shapes:
        p = problem(lattice, samples)
        inp, val, grad, grid = p["inp"], p["val"], p["grad"], p["grid"]
        for order, bound in stencils(dim):
            base = np.asarray(oracle.grid_hess(inp, grid, bound, order, 1))
            for ex in (0, 2):
                tag = (what, lattice, order, bound, ex)
                r = ratio(hess(inp, grid, bound, order, ex), masked_truth("hess", inp, grid, bound, order, ex, base=base), tol, amax(inp))
                assert r <= 1.0, ("hess",) + tag + (r,)
                worst = max(worst, r)
                r = ratio(pushgrad(val, grid, lattice, bound, order, ex), masked_truth("pushgrad", val, grid, bound, order, ex, shape=lattice),
                          tol, amax(val))
                assert r <= 1.0, ("pushgrad",) + tag + (r,)
                worst = max(worst, r)
                if grad_backward is not None:
                    gi, gg = grad_backward(grad, inp, grid, bound, order, ex)
                    wi, wg = masked_truth("grad_backward", inp, grid, bound, order, ex, grad=grad, base=base)
                    r = max(ratio(gi, wi, tol, amax(grad)), ratio(gg, wg, tol, amax(inp, grad)))
                    assert r <= 1.0, ("grad_backward",) + tag + (r,)
                    worst = max(worst, r)
    print("%s, %d-D: worst error / allowed = %.3g" % (what, dim, worst))


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_oracle_mask_identity(dim):
    """The oracle's own masked grid_hess, grid_pushgrad and grid_grad_backward are the identity, to 1e-12 scale."""
    oracle.set_threads(8)
    try:
        _run(dim, SHAPES[dim] + [SMALL[dim]], oracle.grid_hess, oracle.grid_pushgrad, oracle.grid_grad_backward, 1e-12, "oracle")
    finally:
        oracle.set_threads(1)


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_torch_kernels_mask_identity(dim):
    """TorchKernels.hess / .pushgrad -- the product's route for D > 3 and for third order -- are the identity, to 1e-12 scale."""
    oracle.set_threads(8)
    try:
        _run(dim, SHAPES[dim][1:] + [SMALL[dim]],
             lambda inp, grid, b, o, ex: TorchKernels.hess(inp, grid, _pad(b, dim), _pad(o, dim), ex),
             lambda val, grid, shape, b, o, ex: TorchKernels.pushgrad(val, grid, list(shape), _pad(b, dim), _pad(o, dim), ex),
             None, 1e-12, "TorchKernels")
    finally:
        oracle.set_threads(1)


def _pad(codes, dim):
    from interpol.codes import pad_codes
    return pad_codes(codes, dim)
