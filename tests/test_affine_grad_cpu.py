"""The matrix of an `interpol.AffineGrid` is differentiable through grid_pull / grid_push / grid_count.

CPU tensors, float64: the host logic (sepgrid.AffineGrid keeps the autograd link, api routing, the
AffinePull / AffinePush / AffineCount Functions, the create_graph route) on the PyTorch kernel table,
where the gradient of the matrix is obtained by differentiating through `lattice.dense()`.  Runs anywhere.
"""
import pytest
import torch

import interpol

SHP = (11, 9, 10)
OSHP = (8, 10, 7)
# dyadic entries: every coordinate is exact, so `affine_grid`'s matmul and the lattice's own sum give the same numbers
A = [[0.875, 0.125, -0.0625], [-0.125, 1.0625, 0.25], [0.0625, -0.1875, 0.9375]]
T = [1.5, -0.75, 1.125]


def _mat(dim):
    a = torch.tensor(A, dtype=torch.float64)[:dim, :dim]
    t = torch.tensor(T, dtype=torch.float64)[:dim]
    return torch.cat([a, t[:, None]], 1)


def _loss(op, x, grid, shp, kw):
    if op == "pull":
        return interpol.grid_pull(x, grid, **kw).square().sum()
    if op == "push":
        return interpol.grid_push(x, grid, shape=shp, **kw).square().sum()
    return interpol.grid_count(grid, shape=shp, **kw).square().sum()


def _data(op, dim, seed):
    g = torch.Generator().manual_seed(seed)
    shp, oshp = SHP[:dim], OSHP[:dim]
    x = torch.randn([2, 3, *(shp if op == "pull" else oshp)], generator=g, dtype=torch.float64)
    return x, shp, oshp


@pytest.mark.parametrize("dim", [1, 2, 3])
@pytest.mark.parametrize("op", ["pull", "push", "count"])
def test_affine_matrix_receives_a_gradient(op, dim):
    """d loss / d mat through AffineGrid(mat, shape) == through affine_grid(mat, shape), rtol 1e-10."""
    x, shp, oshp = _data(op, dim, 7 + dim)
    for kw in (dict(interpolation=3, bound="dct2", extrapolate=True), dict(interpolation=2, bound="dft", extrapolate=False),
               dict(interpolation=1, bound="replicate", extrapolate=2)):
        mat = _mat(dim).requires_grad_()
        lazy = interpol.AffineGrid(mat, oshp)
        assert lazy.requires_grad
        got, = torch.autograd.grad(_loss(op, x, lazy, shp, kw), mat)
        assert got.shape == (dim, dim + 1)
        mat2 = _mat(dim).requires_grad_()
        want, = torch.autograd.grad(_loss(op, x, interpol.affine_grid(mat2, oshp), shp, kw), mat2)
        assert want.abs().max() > 0
        torch.testing.assert_close(got, want, rtol=1e-10, atol=1e-10 * float(want.abs().max()))


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_affine_matrix_and_image_gradients_together(dim):
    x, shp, oshp = _data("pull", dim, 17)
    kw = dict(interpolation=3, bound="dct2", extrapolate=True)
    x1, m1 = x.clone().requires_grad_(), _mat(dim).requires_grad_()
    gx, gm = torch.autograd.grad(_loss("pull", x1, interpol.AffineGrid(m1, oshp), shp, kw), (x1, m1))
    x2, m2 = x.clone().requires_grad_(), _mat(dim).requires_grad_()
    wx, wm = torch.autograd.grad(_loss("pull", x2, interpol.affine_grid(m2, oshp), shp, kw), (x2, m2))
    torch.testing.assert_close(gx, wx, rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(gm, wm, rtol=1e-10, atol=1e-10 * float(wm.abs().max()))
    # a full (D+1, D+1) matrix: the gradient reaches its first D rows, the last row gets zeros
    full = torch.cat([_mat(dim), torch.zeros(1, dim + 1, dtype=torch.float64)]).requires_grad_()
    gf, = torch.autograd.grad(_loss("pull", x, interpol.AffineGrid(full, oshp), shp, kw), full)
    torch.testing.assert_close(gf[:dim], wm, rtol=1e-10, atol=1e-10 * float(wm.abs().max()))
    assert gf[dim].abs().max() == 0


@pytest.mark.parametrize("dim", [1, 2, 3])
@pytest.mark.parametrize("op", ["pull", "push", "count"])
def test_affine_matrix_gradient_against_finite_differences(op, dim):
    """cubic dct2, extrapolate=True (a cubic spline is C^2): central differences with step 1e-6 agree with every one of
    the D (D+1) analytic entries to 1e-6 of the largest entry."""
    x, shp, oshp = _data(op, dim, 23 + dim)
    kw = dict(interpolation=3, bound="dct2", extrapolate=True)
    mat = _mat(dim).requires_grad_()
    got, = torch.autograd.grad(_loss(op, x, interpol.AffineGrid(mat, oshp), shp, kw), mat)
    h = 1e-6
    fd = torch.zeros_like(got)
    with torch.no_grad():
        for d in range(dim):
            for e in range(dim + 1):
                mp, mm = _mat(dim), _mat(dim)
                mp[d, e] += h
                mm[d, e] -= h
                fd[d, e] = (_loss(op, x, interpol.AffineGrid(mp, oshp), shp, kw)
                            - _loss(op, x, interpol.AffineGrid(mm, oshp), shp, kw)) / (2 * h)
    worst = float((got - fd).abs().max() / got.abs().max())
    print("finite differences", op, dim, "worst error / largest entry: %.3g" % worst)
    assert worst <= 1e-6


@pytest.mark.parametrize("op", ["pull", "push", "count"])
def test_affine_matrix_double_backward(op):
    dim = 2
    x, shp, oshp = _data(op, dim, 31)
    kw = dict(interpolation=3, bound="dct2", extrapolate=True)
    mat = _mat(dim).requires_grad_()
    g1, = torch.autograd.grad(_loss(op, x, interpol.AffineGrid(mat, oshp), shp, kw), mat, create_graph=True)
    assert g1.requires_grad
    g2, = torch.autograd.grad(g1.square().sum(), mat)
    assert g2.shape == (dim, dim + 1) and bool(torch.isfinite(g2).all()) and g2.abs().max() > 0
    # ... and it is the second derivative of the dense route
    mat2 = _mat(dim).requires_grad_()
    w1, = torch.autograd.grad(_loss(op, x, interpol.affine_grid(mat2, oshp), shp, kw), mat2, create_graph=True)
    w2, = torch.autograd.grad(w1.square().sum(), mat2)
    torch.testing.assert_close(g2, w2, rtol=1e-8, atol=1e-8 * float(w2.abs().max()))


def test_affine_grid_grad_goes_through_the_dense_lattice():
    dim = 2
    x, shp, oshp = _data("pull", dim, 41)
    kw = dict(interpolation=3, bound="dct2", extrapolate=True)
    mat = _mat(dim).requires_grad_()
    got, = torch.autograd.grad(interpol.grid_grad(x, interpol.AffineGrid(mat, oshp), **kw).square().sum(), mat)
    mat2 = _mat(dim).requires_grad_()
    out = interpol.grid_grad(x, interpol.affine_grid(mat2, oshp), **kw)
    want, = torch.autograd.grad(out.square().sum(), mat2)
    assert interpol.grid_grad(x, interpol.AffineGrid(mat, oshp), **kw).shape == out.shape
    torch.testing.assert_close(got, want, rtol=1e-10, atol=1e-10 * float(want.abs().max()))


def test_affine_grid_existing_contracts():
    lz = interpol.AffineGrid(_mat(3), OSHP)
    assert lz.requires_grad is False
    assert lz.to(torch.float32).requires_grad is False
    with pytest.raises(ValueError):
        interpol.AffineGrid(torch.zeros(2, 3, 4), OSHP)
    # the learnable lattice stays attached through to(), packed() is a constant
    mat = _mat(3).requires_grad_()
    lg = interpol.AffineGrid(mat, OSHP)
    assert lg.to(torch.float32).requires_grad and not lg.packed(torch.float64).requires_grad
    assert lg.dense().requires_grad
    # forward outputs: bit-identical with and without the gradient
    x, shp, oshp = _data("pull", 3, 5)
    s, _, _ = _data("push", 3, 6)
    for kw in (dict(interpolation=3, bound="dct2", extrapolate=True), dict(interpolation=1, bound="zero", extrapolate=False)):
        assert torch.equal(interpol.grid_pull(x, lg, **kw).detach(), interpol.grid_pull(x, lz, **kw))
        assert torch.equal(interpol.grid_push(s, lg, shape=shp, **kw).detach(), interpol.grid_push(s, lz, shape=shp, **kw))
        assert torch.equal(interpol.grid_count(lg, shape=shp, **kw).detach(), interpol.grid_count(lz, shape=shp, **kw))


def test_affine_push_keeps_the_shape_of_the_lattice():
    """grid_push hands the lattice's own shape to the operator, learnable or not.  A matching lattice gives the same image
    on both paths and a gradient for the matrix; a lattice with a singleton dimension under a larger image is refused by
    the operator's shape check on both paths (the image is broadcast, a lazy lattice is not)."""
    kw = dict(interpolation=1, bound="zero", extrapolate=False)
    g = torch.Generator().manual_seed(3)
    x = torch.randn([2, 3, 8, 10], generator=g, dtype=torch.float64)
    mat = _mat(2).requires_grad_()
    const = interpol.grid_push(x, interpol.AffineGrid(_mat(2), (8, 10)), shape=(9, 11), **kw)
    learn = interpol.grid_push(x, interpol.AffineGrid(mat, (8, 10)), shape=(9, 11), **kw)
    assert learn.shape == (2, 3, 9, 11) and torch.equal(const, learn.detach())
    got, = torch.autograd.grad(learn.square().sum(), mat)
    assert got.shape == (2, 3) and got.abs().max() > 0
    for m in (_mat(2), _mat(2).requires_grad_()):
        with pytest.raises(ValueError, match="same spatial shape"):
            interpol.grid_push(x, interpol.AffineGrid(m, (8, 1)), shape=(9, 11), **kw)


def test_affine_grid_with_a_gradient_refuses_displacement():
    """An AffineGrid holds coordinates.  With a matrix that needs a gradient, displacement=True is refused by all four
    operators instead of dropping the gradient on the way (grid_grad included, which would densify the lattice first)."""
    x, shp, oshp = _data("pull", 2, 43)
    s, _, _ = _data("push", 2, 44)
    lg = interpol.AffineGrid(_mat(2).requires_grad_(), oshp)
    for call in (lambda: interpol.grid_pull(x, lg, displacement=True), lambda: interpol.grid_grad(x, lg, displacement=True),
                 lambda: interpol.grid_push(s, lg, shape=shp, displacement=True),
                 lambda: interpol.grid_count(lg, shape=shp, displacement=True)):
        with pytest.raises(ValueError):
            call()
