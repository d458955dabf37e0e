"""Pins the CPU oracle against the reference's own results, call by call.

Every reference call below is wrapped as `pins(lambda: ...)`: it returns what the
reference (balbasty/torch-interpol @2024_10_08, imported as `interpol_ref`) returned for
that call, stored in tests/golden/golden_pins.npz by
tests/golden/make_golden_pins.py, which runs this module once against the live
reference.  The inputs are seeded and rebuilt here; the lambdas only run then.
Results of more than 64 elements (but the spline weights) are kept as a sample of their values, their
max |ref| and the digest of the oracle output that the recording run compared
with the whole result (tests/golden_util.py: Pins.diff).
"""
import itertools

import numpy as np
import pytest
import torch

from oracle import oracle
from golden_util import Pins

pins = Pins("golden_pins")
P = K = Bound = Spline = None          # the reference's modules: bound only while recording (make_golden_pins.py)


@pytest.fixture(autouse=True)
def _pins(request):
    pins.begin(request.node.name)

SHAPES_IN = (5, 6, 7)
SHAPES_OUT = (4, 3, 5)


def make_case(dim, dtype, seed=0, B=2, C=3):
    g = torch.Generator().manual_seed(seed)
    ishape = SHAPES_IN[:dim]
    oshape = SHAPES_OUT[:dim]
    inp = torch.randn([B, C, *ishape], generator=g, dtype=torch.float64)
    lin = [torch.linspace(-1.0, n, m, dtype=torch.float64) for n, m in zip(ishape, oshape)]
    grid = torch.stack(torch.meshgrid(*lin, indexing="ij"), -1)[None].repeat(B, *([1] * (dim + 1)))
    grid = grid + 1.5 * torch.randn(grid.shape, generator=g, dtype=torch.float64)
    flat = grid.reshape(B, -1, dim)
    # far out-of-bounds samples, exact integers, exact halves
    flat[0, 0] = -3.0 * torch.tensor(ishape, dtype=torch.float64)
    flat[0, 1] = 3.0 * torch.tensor(ishape, dtype=torch.float64) + 0.25
    flat[1, 0] = 2.0
    flat[1, 1] = 1.5
    flat[1, 2] = 0.5
    flat[0, 2] = -0.5
    return inp.to(dtype), grid.to(dtype)


def close(a, b, dtype):
    d, ref_max = pins.diff(a, b)
    scale = max(ref_max, 1e-30)
    tol = 1e-12 if dtype == torch.float64 else 2e-6
    err = d / scale
    assert err <= tol, err


def masked_pushgrad(src4, gin, shape, b, o, extrapolate, dtype):
    """grid_pushgrad under a mask (extrapolate 0 / 2), on the thinned sweep.  The reference carries the mask for pushgrad
    (nd.py:345-347) -- for hess it raises, bug B-2, which is why hess stays at extrapolate = 1 here.  No result of these calls is
    stored: while the module runs against the LIVE reference (tests/golden/make_golden_pins.py binds `P`) the oracle is compared with
    what the reference returns, whole; everywhere it is compared with the reference's own formulation of the mask applied to the
    pinned extrapolate = 1 operator, pushgrad_1(val * inside) (nd.py:10-27, 345-347; tests/test_second_order_cpu.py)."""
    got = oracle.grid_pushgrad(src4, gin, shape, b, o, extrapolate)
    tol = 1e-12 if dtype == torch.float64 else 2e-6
    if P is not None:
        ref = P.grid_pushgrad(src4, gin, shape, b, o, extrapolate)
        assert float((got - ref).abs().max()) <= tol * max(float(ref.abs().max()), 1e-30), (o, b, extrapolate)
    thr = 0.05 if extrapolate == 0 else 0.55
    inside = torch.ones(gin.shape[:-1], dtype=torch.bool)
    for d, n in enumerate(shape):
        inside &= (gin[..., d] > -thr) & (gin[..., d] < n - 1 + thr)
    assert 0 < int(inside.sum()) < inside.numel()
    want = oracle.grid_pushgrad(src4 * inside[:, None, ..., None], gin, shape, b, o, 1)
    assert float((got - want).abs().max()) <= tol * max(float(want.abs().max()), 1e-30), (o, b, extrapolate)


CASES = [(k, b) for k in range(8) for b in range(7)]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("dim", [1, 2, 3])
@pytest.mark.parametrize("extrapolate", [1, 0, 2])
def test_isotropic_sweep(dim, dtype, extrapolate):
    inp, grid = make_case(dim, dtype, seed=dim)
    gin = grid  # push: grid must have input's spatial shape
    for order, bound in CASES:
        if extrapolate != 1 and (order + bound) % 3 != 0:
            continue  # thin the masked sweeps
        b, o = [bound], [order]
        skip_b1 = (order == 0 and dim == 2 and extrapolate != 1)   # reference bug B-1
        if not skip_b1:
            close(oracle.grid_pull(inp, grid, b, o, extrapolate), pins(lambda: P.grid_pull(inp, grid, b, o, extrapolate)), dtype)
        close(oracle.grid_grad(inp, grid, b, o, extrapolate), pins(lambda: P.grid_grad(inp, grid, b, o, extrapolate)), dtype)
        val = inp[..., :1].expand(*inp.shape[:2], *grid.shape[1:-1]) if False else None
        src = torch.randn([inp.shape[0], inp.shape[1], *grid.shape[1:-1]],
                          generator=torch.Generator().manual_seed(7), dtype=torch.float64).to(dtype)
        shape = list(inp.shape[2:])
        close(oracle.grid_push(src, gin, shape, b, o, extrapolate), pins(lambda: P.grid_push(src, gin, shape, b, o, extrapolate)), dtype)
        close(oracle.grid_count(gin, shape, b, o, extrapolate), pins(lambda: P.grid_count(gin, shape, b, o, extrapolate)), dtype)
        src4 = torch.randn([*src.shape, dim], generator=torch.Generator().manual_seed(8),
                           dtype=torch.float64).to(dtype)
        if extrapolate == 1:
            close(oracle.grid_pushgrad(src4, gin, shape, b, o, extrapolate),
                  pins(lambda: P.grid_pushgrad(src4, gin, shape, b, o, extrapolate)), dtype)
            close(oracle.grid_hess(inp, grid, b, o, extrapolate), pins(lambda: P.grid_hess(inp, grid, b, o, extrapolate)), dtype)
        else:
            masked_pushgrad(src4, gin, shape, b, o, extrapolate, dtype)


MIXED = [
    ([2, 3, 5], [2, 5, 0]),
    ([1, 3], [6, 1, 3]),
    ([0, 3], [3]),
    ([3, 1, 2], [4, 2, 6]),
    ([1, 1, 0], [0, 4, 5]),
    ([7, 0, 4], [1, 1, 1]),
]


@pytest.mark.parametrize("dim", [1, 2, 3])
@pytest.mark.parametrize("orders,bounds", MIXED)
def test_mixed_orders_and_bounds(dim, orders, bounds):
    dtype = torch.float64
    inp, grid = make_case(dim, dtype, seed=10 + dim)
    for ex in (1, 0):
        close(oracle.grid_pull(inp, grid, bounds, orders, ex), pins(lambda: P.grid_pull(inp, grid, bounds, orders, ex)), dtype)
        close(oracle.grid_grad(inp, grid, bounds, orders, ex), pins(lambda: P.grid_grad(inp, grid, bounds, orders, ex)), dtype)
        src = torch.randn([inp.shape[0], inp.shape[1], *grid.shape[1:-1]], dtype=dtype,
                          generator=torch.Generator().manual_seed(3))
        shape = list(inp.shape[2:])
        close(oracle.grid_push(src, grid, shape, bounds, orders, ex), pins(lambda: P.grid_push(src, grid, shape, bounds, orders, ex)), dtype)
    close(oracle.grid_hess(inp, grid, bounds, orders, 1), pins(lambda: P.grid_hess(inp, grid, bounds, orders, 1)), dtype)


def test_batch_broadcast():
    inp, grid = make_case(2, torch.float64, seed=5)
    # (the reference operators only broadcast the *grid* batch: nd.py:121-123 expands idx, not inp)
    close(oracle.grid_pull(inp, grid[:1], [3], [3], 1), pins(lambda: P.grid_pull(inp, grid[:1], [3], [3], 1)), torch.float64)
    close(oracle.grid_grad(inp, grid[:1], [6], [2], 1), pins(lambda: P.grid_grad(inp, grid[:1], [6], [2], 1)), torch.float64)
    src = torch.randn([2, 3, *grid.shape[1:-1]], dtype=torch.float64, generator=torch.Generator().manual_seed(6))
    close(oracle.grid_push(src, grid[:1], [5, 6], [3], [3], 1), pins(lambda: P.grid_push(src, grid[:1], [5, 6], [3], [3], 1)), torch.float64)


def test_backward_compositions():
    inp, grid = make_case(3, torch.float64, seed=9)
    inp.requires_grad_(True)
    grid.requires_grad_(True)
    g = torch.Generator().manual_seed(19)
    gout = torch.randn([2, 3, *grid.shape[1:-1]], dtype=torch.float64, generator=g)
    torch.set_grad_enabled(False)   # the reference's *_backward run inside autograd's no-grad backward
    for b, o in (([3], [3]), ([6], [5]), ([1], [1]), ([2, 5, 0], [2, 3, 1])):
        a = oracle.grid_pull_backward(gout, inp, grid, b, o, 1)
        r = pins(lambda: P.grid_pull_backward(gout, inp, grid, b, o, 1))
        close(a[0], r[0], torch.float64)
        close(a[1], r[1], torch.float64)
    src = torch.randn([2, 3, *grid.shape[1:-1]], dtype=torch.float64, generator=g).requires_grad_(True)
    gvol = torch.randn([2, 3, 5, 6, 7], dtype=torch.float64, generator=g)
    a = oracle.grid_push_backward(gvol, src, grid, [3], [3], 1)
    r = pins(lambda: P.grid_push_backward(gvol, src, grid, [3], [3], 1))
    close(a[0], r[0], torch.float64)
    close(a[1], r[1], torch.float64)
    a = oracle.grid_count_backward(gvol[:, :1], grid, [3], [3], 1)
    r = pins(lambda: P.grid_count_backward(gvol[:, :1], grid, [3], [3], 1))
    close(a, r, torch.float64)
    gg = torch.randn([2, 3, *grid.shape[1:-1], 3], dtype=torch.float64, generator=g)
    a = oracle.grid_grad_backward(gg, inp, grid, [3], [3], 1)
    r = pins(lambda: P.grid_grad_backward(gg, inp, grid, [3], [3], 1))
    close(a[0], r[0], torch.float64)
    close(a[1], r[1], torch.float64)
    torch.set_grad_enabled(True)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_prefilter(dtype):
    g = torch.Generator().manual_seed(42)
    for n in (1, 2, 3, 7, 9, 11, 64, 200):
        x = torch.randn([3, n, 4], generator=g, dtype=torch.float64).to(dtype)
        for order in range(0, 8):
            for bound in (0, 1, 2, 3, 6):
                ref = pins(lambda: K.spline_coeff(x, bound, order, dim=1))
                got = oracle.spline_coeff(x, bound, order, dim=1)
                d, ref_max = pins.diff(got, ref)
                tol = 1e-11 if dtype == torch.float64 else 5e-5
                assert d <= tol * max(1.0, ref_max), (n, order, bound)
    x = torch.randn([2, 9, 10, 11], generator=g, dtype=torch.float64)
    ref = pins(lambda: K.spline_coeff_nd(x, [2, 3, 6], [2, 3, 5], 3))
    got = oracle.spline_coeff_nd(x, [2, 3, 6], [2, 3, 5], 3)
    assert pins.diff(got, ref)[0] < 1e-11
    with pytest.raises(NotImplementedError):
        oracle.spline_coeff(x, 5, 3, dim=-1)


def test_index_and_sign_tables():
    for n in (1, 2, 3, 4, 7):
        i = torch.arange(-4 * n - 3, 4 * n + 4)
        for b in range(7):
            idx = pins(lambda: Bound(b).index(i, n)).tolist()
            sgn = pins(lambda: Bound(b).transform(i, n))
            for ii, want in zip(i.tolist(), idx):
                assert oracle.bound_index(b, ii, n) == want, (b, n, ii)
            for k, ii in enumerate(i.tolist()):
                got = oracle.bound_sign(b, ii, n)
                if sgn is None:
                    assert got is None
                else:
                    assert got == int(sgn[k]), (b, n, ii)


def test_weights_bitexact_fp32():
    for k in range(8):
        half = (k + 1) / 2
        x = torch.linspace(-half, half, 4001, dtype=torch.float32)[::7]
        w, g, h = pins(lambda: (Spline(k).fastweight(x), Spline(k).fastgrad(x), Spline(k).fasthess(x)), whole=True)
        for j in range(len(x)):
            xv = float(x[j])
            assert oracle.weight(k, xv, "f32") == float(w[j]), (k, xv)
            assert oracle.wgrad(k, xv, "f32") == float(g[j]), (k, xv)
            assert oracle.whess(k, xv, "f32") == float(h[j]), (k, xv)
