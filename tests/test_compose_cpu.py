"""`interpol.compose` / `interpol.exp` without a GPU: CPU tensors and 4-D fields run the composed expression

    right + grid_pull(left.movedim(-1, -D-1), right, displacement=True).movedim(-D-1, -1)

over the package's PyTorch kernel table.  The reference's answer -- `right + interpol_ref.grid_pull(left channel-first,
add_identity_grid(right))`, float64 -- is read from tests/golden/golden_compose.npz (recorded by
tests/golden/make_golden_compose.py from the live reference, which does not travel).

Displacements are multiples of 1/64 with |.| <= 6, so every coordinate o + right is exact in float32 and float64 alike.
"""
import os

import numpy as np
import pytest
import torch

import interpol
from interpol import ops

HERE = os.path.dirname(os.path.abspath(__file__))
BOUNDS = ["zero", "replicate", "dct1", "dct2", "dst1", "dst2", "dft"]


def dyadic(gen, shape, amp=6, dtype=torch.float64):
    """multiples of 1/64 in [-amp, amp]"""
    return torch.randint(-64 * amp, 64 * amp + 1, shape, generator=gen).to(dtype) / 64


def composed(left, right, **kw):
    """The definition, through the public grid_pull."""
    dim = right.shape[-1]
    return right + interpol.grid_pull(left.movedim(-1, -dim - 1), right, displacement=True, **kw).movedim(-dim - 1, -1)


def fields(dim, seed, dtype=torch.float64, B=2, lB=None):
    gen = torch.Generator().manual_seed(seed)
    lshape, oshape = ((67,), (130,)) if dim == 1 else (((13, 22), (19, 11)) if dim == 2 else ((13, 10, 17), (11, 14, 9)))
    left = torch.randn([B if lB is None else lB, *lshape, dim], generator=gen, dtype=dtype)
    right = dyadic(gen, [B, *oshape, dim], dtype=dtype)
    return left, right


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_compose_on_cpu_is_the_composed_expression(dim):
    left, right = fields(dim, 10 + dim)
    for order, bound, ex in ((1, "dft", True), (3, "dct2", False), (2, "zero", 2), (0, "replicate", True), (5, "dct1", True)):
        kw = dict(interpolation=order, bound=bound, extrapolate=ex)
        assert not ops.compose_covered(left, right, [order])
        got = interpol.compose(left, right, **kw)
        assert got.shape == right.shape and got.dtype == right.dtype
        assert torch.equal(got, composed(left, right, **kw)), (dim, order, bound, ex)
    # defaults: linear, dft, extrapolate
    assert torch.equal(interpol.compose(left, right), composed(left, right, interpolation=1, bound="dft", extrapolate=True))
    # a mixed per-dim list
    if dim == 3:
        kw = dict(interpolation=[1, 2, 3], bound=["dct2", "dft", "zero"], extrapolate=True)
        assert torch.equal(interpol.compose(left, right, **kw), composed(left, right, **kw))


def test_compose_broadcasts_and_folds_batches():
    left, right = fields(2, 3, lB=1)
    want = composed(left.expand(2, -1, -1, -1), right, interpolation=1, bound="dft", extrapolate=True)
    assert torch.equal(interpol.compose(left, right), want)
    assert torch.equal(interpol.compose(left[0], right), want)                       # no batch on the left
    assert torch.equal(interpol.compose(left[0], right[0]), want[0])                 # no batch at all
    stacked = right.reshape(2, 1, *right.shape[1:]).expand(2, 3, *right.shape[1:])
    got = interpol.compose(left[0], stacked)                                        # two leading dims
    assert got.shape == stacked.shape and torch.equal(got[:, 1], want)
    # right broadcast over left's batch
    l2, r2 = fields(2, 4)
    got = interpol.compose(l2, r2[:1])
    assert torch.equal(got, composed(l2, r2[:1].expand(2, -1, -1, -1), interpolation=1, bound="dft", extrapolate=True))


def test_compose_and_exp_on_a_4d_field():
    gen = torch.Generator().manual_seed(44)
    shape = (4, 5, 3, 4)
    left = torch.randn([2, *shape, 4], generator=gen, dtype=torch.float64)
    right = dyadic(gen, [2, 3, 4, 2, 3, 4], amp=2)
    kw = dict(interpolation=1, bound="dft", extrapolate=True)
    assert not ops.compose_covered(left, right, [1])
    assert torch.equal(interpol.compose(left, right, **kw), composed(left, right, **kw))
    vel = dyadic(gen, [1, *shape, 4], amp=2)
    u = vel * 0.25
    for _ in range(2):
        u = composed(u, u, **kw)
    assert torch.equal(interpol.exp(vel, 2, **kw), u)


@pytest.mark.parametrize("dim", [2, 3])
def test_compose_agrees_with_the_recorded_reference(dim):
    z = np.load(os.path.join(HERE, "golden", "golden_compose.npz"))
    left = torch.as_tensor(z["d%d_left" % dim]).double()
    right = torch.as_tensor(z["d%d_right" % dim]).double()
    k = 0
    while "d%d_c%d_want" % (dim, k) in z.files:
        order, bound, ex = (int(v) for v in z["d%d_c%d_case" % (dim, k)])
        want = torch.as_tensor(z["d%d_c%d_want" % (dim, k)])
        got = interpol.compose(left, right, interpolation=order, bound=BOUNDS[bound], extrapolate=ex)
        pulled = (want - right).abs().max()
        err = (got - want).abs()
        assert bool((err <= 1e-11 * want.abs() + 1e-11 * pulled).all()), (dim, order, bound, ex, float(err.max()))
        k += 1
    assert k >= 2


def test_exp_on_cpu():
    gen = torch.Generator().manual_seed(5)
    vel = dyadic(gen, [2, 9, 8, 7, 3], amp=2)
    kw = dict(interpolation=1, bound="dft", extrapolate=True)
    assert torch.equal(interpol.exp(vel, steps=0), vel)
    assert torch.equal(interpol.exp(vel, steps=0, inverse=True), -vel)
    u = vel * 2.0 ** -3
    for _ in range(3):
        u = interpol.compose(u, u, **kw)
    assert torch.equal(interpol.exp(vel, 3), u)
    assert torch.equal(interpol.exp(vel, 3, inverse=True), interpol.exp(-vel, 3))
    # with a graph: the same values, and a gradient that matches the composed expression's
    v = vel.clone().requires_grad_()
    y = interpol.exp(v, 3, interpolation=3, bound="dct2")
    g, = torch.autograd.grad(y.square().sum(), v)
    v2 = vel.clone().requires_grad_()
    u = v2 * 2.0 ** -3
    for _ in range(3):
        u = composed(u, u, interpolation=3, bound="dct2", extrapolate=True)
    g2, = torch.autograd.grad(u.square().sum(), v2)
    assert torch.equal(y.detach(), u.detach())
    assert float((g - g2).abs().max()) <= 1e-11 * float(g2.abs().max())
    with pytest.raises(ValueError):
        interpol.exp(vel, steps=-1)


def test_compose_gradients_on_cpu():
    left, right = fields(2, 8, lB=1)
    kw = dict(interpolation=3, bound="dct2", extrapolate=True)
    w = torch.randn(right.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    res = []
    for f in (interpol.compose, composed):
        l, r = left.clone().requires_grad_(), right.clone().requires_grad_()
        res.append(torch.autograd.grad((f(l, r, **kw) * w).sum(), (l, r)))
    for a, b in zip(*res):
        assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-11 * float(b.abs().max())
    # double backward through the composed Functions
    res = []
    for f in (interpol.compose, composed):
        l, r = left.clone().requires_grad_(), right.clone().requires_grad_()
        g1, = torch.autograd.grad(f(l, r, **kw).square().sum(), r, create_graph=True)
        res.append(torch.autograd.grad(g1.square().sum(), (l, r)))
    for a, b in zip(*res):
        assert float((a - b).abs().max()) <= 1e-9 * float(b.abs().max())


def test_compose_refuses_bad_fields():
    f = torch.zeros(2, 5, 6, 2)
    with pytest.raises(ValueError):
        interpol.compose(f, f.double())                                  # mismatched dtypes
    with pytest.raises(ValueError):
        interpol.compose(torch.zeros(5, 6, 3), torch.zeros(5, 6, 3))     # last dim 3, two spatial dims
    with pytest.raises(ValueError):
        interpol.compose(torch.zeros(2, 5, 6, 3), f)                     # left's components do not match right's
    with pytest.raises(ValueError):
        interpol.compose(torch.zeros(5, 6, 0), torch.zeros(5, 6, 0))     # D = 0
    with pytest.raises(ValueError):
        interpol.exp(torch.zeros(5, 6, 0))
    with pytest.raises(ValueError):
        interpol.compose(f.long(), f.long())
