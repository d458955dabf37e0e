"""Gradient of the matrix of an `interpol.AffineGrid` on the device (csrc/affine_grad.hip).

Truth everywhere: the float64 DENSE route on the device -- `affine_grid(mat, shape)`, the existing operator, torch autograd
down to `mat` -- which also yields the per-sample grid gradient g(b, o) the allowance is made of:

    |got - want|[d, e] <= tol * sum_{b,o} (|g_d(b,o)| + max |g_d|) * o_e          (o_D = 1)

the project's bar for a grid gradient (relative to its largest entry, plus relative to the entry itself) applied per
sample and summed; tol = 1e-5 for float32 images, 1e-11 for float64, 1e-2 for bf16 / f16 storage.  g never comes from the
code under test.  The matrix entries are dyadic: every coordinate is exact in float32, so both precisions see the same
`floor` and the same mask and the piecewise-constant gradients of orders 0 and 1 cannot flip between the two sides.
"""
import ctypes

import numpy as np
import pytest
import torch

import interpol
from interpol import _hip
from oracle import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHP = (41, 36, 44)
OSHP = (37, 40, 35)
A = [[0.875, 0.125, -0.0625], [-0.125, 1.0625, 0.25], [0.0625, -0.1875, 0.9375]]
T = [2.5, -1.75, 3.125]
# (bound, order, extrapolate): the five of test_affine_grid_in_kernel_matches_oracle_on_dense_affine_grid, order 7, one mixed
CASES = ((3, 3, 1), (6, 2, 0), (1, 1, 2), (4, 3, 1), (0, 5, 1), (3, 7, 1), (3, [1, 2, 3], 1))
TOL = {torch.float32: 1e-5, torch.float64: 1e-11, torch.bfloat16: 1e-2, torch.float16: 1e-2}


def _mat(dim, dtype=torch.float32):
    a = torch.tensor(A, dtype=dtype)[:dim, :dim]
    t = torch.tensor(T, dtype=dtype)[:dim]
    return torch.cat([a, t[:, None]], 1)


def _codes(dim, bound, order):
    return [bound] * dim, (list(order[:dim]) if isinstance(order, list) else [order] * dim)


def _index(oshp, dtype=torch.float64, device=DEV):
    """(N, D+1): the integer index of every sample, and 1"""
    o = interpol.identity_grid(oshp, dtype=dtype, device=device).reshape(-1, len(oshp))
    return torch.cat([o, o.new_ones([o.shape[0], 1])], 1)


def _truth(op, a, v, mat, shp, oshp, b, o, ex):
    """float64 dense route.  pull: a = grad_out (B,C,*oshp), v = vol (B,C,*shp); push: a = val (B,C,*oshp), v = grad_vol_out
    (B,C,*shp); count: a None.  -> (want (D,D+1), allowance per unit of tol (D,D+1))"""
    dim = len(oshp)
    B = v.shape[0]
    m = mat.to(DEV, torch.float64).requires_grad_()
    dense = interpol.affine_grid(m, oshp)[None].expand(B, *oshp, dim)
    kw = dict(interpolation=o, bound=b, extrapolate=ex)
    v64 = v.to(DEV, torch.float64)
    if op == "pull":
        loss = (interpol.grid_pull(v64, dense, **kw) * a.to(DEV, torch.float64)).sum()
    elif op == "push":
        loss = (interpol.grid_push(a.to(DEV, torch.float64), dense, shape=list(shp), **kw) * v64).sum()
    else:
        loss = (interpol.grid_count(dense, shape=list(shp), **kw) * v64).sum()
    want, g = torch.autograd.grad(loss, (m, dense))
    g = g.reshape(B, -1, dim)
    weight = (g.abs() + g.abs().amax(dim=(0, 1), keepdim=True)).sum(0)             # (N, D)
    return want, weight.t() @ _index(oshp)


def _check(got, want, allow, tol, what):
    err = (got.double() - want).abs()
    ratio = float((err / (tol * allow).clamp_min(1e-300)).max())
    print("affine grad", what, "worst error / allowance: %.3g" % ratio)
    assert bool(torch.isfinite(got).all()), what
    assert ratio <= 1.0, (what, ratio, got, want)


def _inputs(dim, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    shp, oshp = SHP[:dim], OSHP[:dim]
    vol = torch.randn([2, 3, *shp], generator=g).to(dtype)               # (16-bit: the reference sees the rounded values)
    src = torch.randn([2, 3, *oshp], generator=g).to(dtype)
    return vol, src, shp, oshp


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16, torch.float16], ids=["f32", "f64", "bf16", "f16"])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_affine_grad_mat_matches_the_dense_route(dim, dtype):
    vol, src, shp, oshp = _inputs(dim, dtype, 90 + dim)
    gdt = torch.float64 if dtype == torch.float64 else torch.float32
    lazy = interpol.AffineGrid(_mat(dim, gdt), oshp).to(DEV)
    assert torch.equal(lazy.dense().cpu(), interpol.affine_grid(_mat(dim, gdt), oshp)[None])     # exact products
    v, s = vol.to(DEV), src.to(DEV)
    for bound, order, ex in CASES:
        b, o = _codes(dim, bound, order)
        what = (dim, str(dtype), bound, order, ex)
        got = _hip.affine_pull_backward(s, v, lazy, b, o, ex)
        assert got.shape == (dim, dim + 1) and got.dtype == gdt
        _check(got, *_truth("pull", src, vol, _mat(dim), shp, oshp, b, o, ex), TOL[dtype], ("pull",) + what)
        got = _hip.affine_push_backward(v, s, lazy, b, o, ex)
        _check(got, *_truth("push", src, vol, _mat(dim), shp, oshp, b, o, ex), TOL[dtype], ("push",) + what)
        got = _hip.affine_push_backward(v[:, :1], None, lazy, b, o, ex)
        _check(got, *_truth("count", None, vol[:, :1], _mat(dim), shp, oshp, b, o, ex), TOL[dtype], ("count",) + what)


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_affine_grad_mat_matches_the_c_oracle(dim):
    """The C oracle's grid_pull_backward grid gradient, contracted with the sample index in numpy."""
    vol, src, shp, oshp = _inputs(dim, torch.float64, 190 + dim)
    b, o, ex = [3] * dim, [3] * dim, 1
    dn = interpol.affine_grid(_mat(dim, torch.float64), oshp)[None].expand(2, *oshp, dim).contiguous().numpy()
    _, gg = oracle.grid_pull_backward(src.numpy(), vol.numpy(), dn, b, o, ex)
    gg = np.asarray(gg).reshape(2, -1, dim)
    idx = _index(oshp, device="cpu").numpy()
    want = torch.as_tensor(np.einsum("bnd,ne->de", gg, idx))
    allow = torch.as_tensor(np.einsum("nd,ne->de", (np.abs(gg) + np.abs(gg).max(axis=(0, 1), keepdims=True)).sum(0), idx))
    for dtype in (torch.float64, torch.float32):
        lazy = interpol.AffineGrid(_mat(dim, dtype), oshp).to(DEV)
        got = _hip.affine_pull_backward(src.to(DEV, dtype), vol.to(DEV, dtype), lazy, b, o, ex).cpu()
        _check(got, want, allow, TOL[dtype], ("oracle pull", dim, str(dtype)))


def test_affine_grad_mat_is_deterministic():
    """No atomics, a fixed summation order: the same call twice gives the same bits (f32, 3-D cubic, 2 x 3 x 41 x 36 x 44)."""
    g = torch.Generator().manual_seed(7)
    shape = (41, 36, 44)
    vol = torch.randn([2, 3, *shape], generator=g).to(DEV)
    src = torch.randn([2, 3, *shape], generator=g).to(DEV)
    lazy = interpol.AffineGrid(_mat(3), shape).to(DEV)
    b, o = [3] * 3, [3] * 3
    first = (_hip.affine_pull_backward(src, vol, lazy, b, o, 1), _hip.affine_push_backward(vol, src, lazy, b, o, 1),
             _hip.affine_push_backward(vol[:, :1], None, lazy, b, o, 1))
    other = torch.randn(1 << 22, device=DEV).sum()                                   # (something else on the device in between)
    again = (_hip.affine_pull_backward(src, vol, lazy, b, o, 1), _hip.affine_push_backward(vol, src, lazy, b, o, 1),
             _hip.affine_push_backward(vol[:, :1], None, lazy, b, o, 1))
    assert bool(torch.isfinite(other))
    for a, c in zip(first, again):
        assert torch.equal(a, c) and float(a.abs().max()) > 0


@pytest.mark.parametrize("op", ["pull", "push", "count"])
def test_affine_grad_mat_through_the_api(op):
    """mat.grad through interpol.grid_pull / grid_push / grid_count: with x.grad, and alone (needs_input_grad skipping)."""
    dim = 3
    vol, src, shp, oshp = _inputs(dim, torch.float32, 33)
    kw = dict(interpolation=3, bound="dct2", extrapolate=True)
    b, o, ex = [3] * dim, [3] * dim, 1
    if op == "pull":
        x0, w, truth = vol, src, _truth("pull", src, vol, _mat(dim), shp, oshp, b, o, ex)
    elif op == "push":
        x0, w, truth = src, vol, _truth("push", src, vol, _mat(dim), shp, oshp, b, o, ex)
    else:
        x0, w, truth = None, vol[:1, :1], _truth("count", None, vol[:1, :1], _mat(dim), shp, oshp, b, o, ex)
    w = w.to(DEV)

    def run(x, mat):
        lz = interpol.AffineGrid(mat, oshp)
        assert lz.requires_grad
        if op == "pull":
            y = interpol.grid_pull(x, lz, **kw)
        elif op == "push":
            y = interpol.grid_push(x, lz, shape=shp, **kw)
        else:
            y = interpol.grid_count(lz, shape=shp, **kw)[None, None]
        return (y * w).sum()

    mat = _mat(dim).to(DEV).requires_grad_()
    run(None if x0 is None else x0.to(DEV), mat).backward()
    _check(mat.grad, *truth, 1e-5, ("api", op, "mat alone"))
    alone = mat.grad.clone()
    if x0 is not None:
        mat = _mat(dim).to(DEV).requires_grad_()
        x = x0.to(DEV).requires_grad_()
        run(x, mat).backward()
        assert torch.equal(mat.grad, alone)
        # the image gradient is the one of the constant lattice
        x2 = x0.to(DEV).requires_grad_()
        lz = interpol.AffineGrid(_mat(dim).to(DEV), oshp)
        y = interpol.grid_pull(x2, lz, **kw) if op == "pull" else interpol.grid_push(x2, lz, shape=shp, **kw)
        (y * w).sum().backward()
        assert float((x.grad - x2.grad).abs().max()) <= 1e-5 * float(x2.grad.abs().max())
    # under autocast the Functions run in float32, like the dense ones
    mat = _mat(dim).to(DEV).requires_grad_()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = run(None if x0 is None else x0.to(DEV), mat)
    loss.backward()
    assert mat.grad.dtype == torch.float32
    _check(mat.grad, *truth, 1e-5, ("api", op, "autocast"))


def test_affine_grad_mat_double_backward_on_the_device():
    dim = 2
    vol, src, shp, oshp = _inputs(dim, torch.float64, 51)
    kw = dict(interpolation=3, bound="dct2", extrapolate=True)
    v = vol.to(DEV)
    res = []
    for lattice in (lambda m: interpol.AffineGrid(m, oshp), lambda m: interpol.affine_grid(m, oshp)):
        m = _mat(dim, torch.float64).to(DEV).requires_grad_()
        g1, = torch.autograd.grad(interpol.grid_pull(v, lattice(m), **kw).square().sum(), m, create_graph=True)
        g2, = torch.autograd.grad(g1.square().sum(), m)
        res.append(g2)
    assert bool(torch.isfinite(res[0]).all())
    assert float((res[0] - res[1]).abs().max()) <= 1e-8 * float(res[1].abs().max())


def test_affine_grad_mat_in_a_captured_graph():
    """The pair of launches has no host synchronisation: captured once, replayed on new data."""
    gen = torch.Generator().manual_seed(79)
    n = 48
    shape = (n, n, n)
    vol = torch.randn([2, 2, *shape], generator=gen).to(DEV)
    src = torch.randn([2, 2, *shape], generator=gen).to(DEV)
    mat = _mat(3).to(DEV)
    lazy = interpol.AffineGrid(mat, shape)
    b, o = [3] * 3, [3] * 3

    def calls():
        return (_hip.affine_pull_backward(src, vol, lazy, b, o, 1), _hip.affine_push_backward(vol, src, lazy, b, o, 1))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        calls()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = calls()
    for it in range(2):
        g.replay()
        torch.cuda.synchronize()
        first = [t.clone() for t in out]
        g.replay()
        torch.cuda.synchronize()
        eager = calls()
        for a, f, e in zip(out, first, eager):
            assert torch.equal(a, f) and torch.equal(a, e), it
        vol.copy_(torch.randn(vol.shape, generator=gen))
        src.copy_(torch.randn(src.shape, generator=gen))
    assert not torch.equal(first[0], _hip.affine_pull_backward(src, vol, lazy, b, o, 1))


def test_affine_grad_entry_points_validate_before_launching():
    L = _hip.lib()
    dim, shp = 3, (12, 12, 12)
    vol = torch.randn(1, 1, *shp, device=DEV)
    gout = torch.randn(1, 1, *shp, device=DEV)
    mat = _mat(3).to(DEV).contiguous()
    st = [vol.stride(0), vol.stride(1), *vol.stride()[2:]]
    vs = st + [0, 0]

    def problem(flags):
        return _hip.make_problem(dim, torch.float32, torch.float32, [3] * 3, [3] * 3, 1, 1, 1, shp, shp, st, [0] * 5, vs, flags)

    sentinel = 12345.0
    gmat = torch.full([3, 4], sentinel, device=DEV)
    p = problem(_hip.FLAG_AFFINE_GRID)
    need = int(L.interpol_affine_backward_workspace(ctypes.byref(p)))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    args = lambda t: ctypes.c_void_p(t.data_ptr())
    null = ctypes.c_void_p(0)
    # without the affine flag: INTERPOL_E_STRIDE (-10), from all three
    q = problem(0)
    for i, v in enumerate([3 * 12 ** 3, 3 * 12 ** 2, 3 * 12, 3, 1]):          # (a dense (1, 12, 12, 12, 3) grid's strides)
        q.grid_stride[i] = v
    assert int(L.interpol_affine_backward_workspace(ctypes.byref(q))) == -10
    assert L.interpol_pull_backward_affine(ctypes.byref(q), args(gout), args(vol), args(mat), args(gmat), args(ws), need, null) == -10
    assert L.interpol_push_backward_affine(ctypes.byref(q), args(gout), args(vol), args(mat), args(gmat), args(ws), need, null) == -10
    assert L.interpol_push_backward_affine(ctypes.byref(q), args(gout), null, args(mat), args(gmat), args(ws), need, null) == -10
    # an undersized workspace: a negative code, nothing launched
    assert L.interpol_pull_backward_affine(ctypes.byref(p), args(gout), args(vol), args(mat), args(gmat), args(ws), need - 8, null) < 0
    assert L.interpol_push_backward_affine(ctypes.byref(p), args(gout), args(vol), args(mat), args(gmat), args(ws), 0, null) < 0
    assert L.interpol_pull_backward_affine(ctypes.byref(p), args(gout), args(vol), args(mat), args(gmat), null, need, null) < 0
    torch.cuda.synchronize()
    assert bool((gmat == sentinel).all())
    # the per-sample grid gradient of an affine lattice is still refused by the dense entry points
    with pytest.raises(RuntimeError):
        _hip.pull_backward(gout, vol, interpol.AffineGrid(mat, shp), [3] * 3, [3] * 3, 1, False, True)
    # ... and the same call with everything in place runs
    assert L.interpol_pull_backward_affine(ctypes.byref(p), args(gout), args(vol), args(mat), args(gmat), args(ws), need, null) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(gmat).all()) and not bool((gmat == sentinel).any())


def test_affine_registration_step_at_size():
    """1 x 1 x 128^3 float32, cubic dct2: 20 steps of plain gradient descent on the 12 entries, from the identity, towards a
    known small dyadic affine.  The step is 1 / trace of the Gauss-Newton Hessian of the mean squared error at the identity,
    2 mean_o |grad I(o)|^2 (|o|^2 + 1) -- an upper bound of its largest eigenvalue, computed from the fixed image alone --
    so every step must decrease the error; the fused route and the dense route must arrive at the same error."""
    n = 128
    shape = (n, n, n)
    gen = torch.Generator().manual_seed(5)
    coarse = torch.randn([1, 1, 16, 16, 16], generator=gen)
    fixed = torch.nn.functional.interpolate(coarse, size=shape, mode="trilinear", align_corners=True).to(DEV)
    kw = dict(interpolation=3, bound="dct2", extrapolate=True)
    true = torch.eye(3, 4) + torch.tensor([[1 / 64, 1 / 128, 0, 0.5], [-1 / 128, -1 / 64, 1 / 256, -0.25], [0, 1 / 128, 1 / 64, 0.375]])
    moving = interpol.grid_pull(fixed, interpol.AffineGrid(true.to(DEV), shape), **kw)
    gI = interpol.grid_grad(fixed, interpol.AffineGrid(torch.eye(3, 4).to(DEV), shape), **kw)[0, 0].double()   # (*shape, 3)
    o2 = interpol.identity_grid(shape, dtype=torch.float64, device=DEV).square().sum(-1) + 1
    lr = 1.0 / float(2 * (gI.square().sum(-1) * o2).mean())

    def descend(lattice):
        mat = torch.eye(3, 4, device=DEV).requires_grad_()
        losses = []
        for _ in range(20):
            loss = (interpol.grid_pull(fixed, lattice(mat), **kw) - moving).double().square().mean()   # (the mean of 2 M squares: in double)
            g, = torch.autograd.grad(loss, mat)
            losses.append(float(loss))
            mat = (mat.detach() - lr * g).requires_grad_()
        with torch.no_grad():
            losses.append(float((interpol.grid_pull(fixed, lattice(mat), **kw) - moving).double().square().mean()))
        return losses

    fused = descend(lambda m: interpol.AffineGrid(m, shape))
    dense = descend(lambda m: interpol.affine_grid(m, shape))
    print("registration: fused", ["%.6g" % v for v in fused])
    print("registration: dense", ["%.6g" % v for v in dense])
    assert all(b < a for a, b in zip(fused[:-1], fused[1:])), fused
    assert abs(fused[-1] - dense[-1]) <= 1e-4 * dense[-1], (fused[-1], dense[-1])
