"""`interpol.ssd_gauss_newton_affine`: the composed form (`torch_kernels.ssd_gauss_newton_affine_composed`) in float64 on tiny
lattices, against autograd through `affine_grid` + `grid_pull`; the helpers that tests/test_ssd_affine_gpu.py shares.

gradient = d loss / d mat[:D] and hessian = J^T W J with J the Jacobian of the residuals with respect to mat[:D]: both to 1e-10
relative to the largest entry (observed: a few 1e-16).  The recovery problem: six Gaussian blobs on 24 x 20 x 22, the fixed image
their pull through a known dyadic matrix on 20 x 22 x 18, ten plain Gauss-Newton iterations from the identity.
"""
import itertools

import pytest
import torch

import interpol
from interpol import backend, ops, torch_kernels

CASES = [((5, 4, 6), (4, 5, 3)), ((7, 4), (6, 5)), ((7,), (9,))]          # moving -> fixed
IDS = ["x".join(map(str, s)) for _, s in CASES]
# dyadic entries, multiples of 1/32: every coordinate is exact in float32
MATS = {
    3: [[0.875, 0.125, -0.0625, 2.53125], [-0.125, 1.0625, 0.25, -1.71875], [0.0625, -0.1875, 0.9375, 3.09375]],
    2: [[0.9375, 0.125, 1.28125], [-0.1875, 1.0625, -0.84375]],
    1: [[0.875, 2.53125]],
}


def matrix(dim, dtype=torch.float64, scale=1.0):
    """the dyadic matrix of `dim` dimensions; scale: its translation times `scale` (stays dyadic for a dyadic scale)"""
    m = torch.tensor(MATS[dim], dtype=dtype)
    m[:, -1] *= scale
    return m


def problem(inshape, shape, seed, dtype=torch.float64, C=2, B=None, weighted=True):
    """moving (B?, C, *inshape), fixed (B?, C, *shape), weight (B?, *shape) | None: i.i.d. normal images, uniform weights"""
    gen = torch.Generator().manual_seed(seed)
    lead = [] if B is None else [B]
    moving = torch.randn(*lead, C, *inshape, generator=gen, dtype=torch.float64).to(dtype)
    fixed = torch.randn(*lead, C, *shape, generator=gen, dtype=torch.float64).to(dtype)
    weight = torch.rand(*lead, *shape, generator=gen, dtype=torch.float64).to(dtype) if weighted else None
    return moving, fixed, weight


def residuals(moving, fixed, mat, shape, **kw):
    return interpol.grid_pull(moving, interpol.affine_grid(mat, shape), **kw) - fixed


def autograd_truth(moving, fixed, mat, weight, **kw):
    """(loss, d loss / d mat, J^T W J) by autograd through affine_grid and grid_pull; unbatched float64 operands"""
    shape, dim = list(fixed.shape[1:]), mat.shape[-1] - 1
    w = torch.ones(shape, dtype=fixed.dtype) if weight is None else weight
    m = mat.clone().requires_grad_(True)
    r = residuals(moving, fixed, m, shape, **kw)
    loss = 0.5 * (w * r * r).sum()
    grad, = torch.autograd.grad(loss, m)
    J = torch.autograd.functional.jacobian(lambda a: residuals(moving, fixed, a, shape, **kw), mat).reshape(-1, dim * (dim + 1))
    W = w.expand(fixed.shape).reshape(-1, 1)
    return loss.detach(), grad, J.T @ (W * J)


def close(got, want, rel=1e-10):
    return float((got - want).abs().max()) <= rel * max(float(want.abs().max()), 1e-300)


@pytest.mark.parametrize("extrapolate", [True, False], ids=["extrapolate", "in_view"])
@pytest.mark.parametrize("bound", ["dct2", "dft", "zero"])
@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_gradient_and_hessian_are_those_of_autograd(case, order, bound, extrapolate):
    inshape, shape = CASES[case]
    dim = len(shape)
    for C in (1, 2):
        moving, fixed, weight = problem(inshape, shape, 10 * case + C, C=C, weighted=C == 2)
        mat = matrix(dim, scale=0.25)
        kw = dict(interpolation=order, bound=bound, extrapolate=extrapolate)
        loss, grad, hess = interpol.ssd_gauss_newton_affine(moving, fixed, mat, weight, **kw)
        tl, tg, th = autograd_truth(moving, fixed, mat, weight, **kw)
        P = dim * (dim + 1)
        assert loss.shape == () and grad.shape == (dim, dim + 1) and hess.shape == (P, P)
        assert close(loss, tl) and close(grad, tg) and close(hess, th), (float((grad - tg).abs().max()), float((hess - th).abs().max()))
        assert torch.equal(hess, hess.mT)
        ev = torch.linalg.eigvalsh(hess)
        assert float(ev[0]) >= -1e-10 * float(ev[-1])
        l2, g2, h2 = interpol.ssd_gauss_newton_affine(moving, fixed, mat, weight, hessian=False, **kw)
        assert h2 is None and torch.equal(l2, loss) and torch.equal(g2, grad)


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_a_batch_of_matrices_is_one_call_per_matrix(case):
    inshape, shape = CASES[case]
    dim = len(shape)
    moving, fixed, weight = problem(inshape, shape, 70 + case, B=3)
    mats = torch.stack([matrix(dim, scale=s) for s in (0.25, 0.5, -0.125)])
    mats[1, 0, 0] += 0.0625
    kw = dict(interpolation=3, bound="dct2", extrapolate=False)
    got = interpol.ssd_gauss_newton_affine(moving, fixed, mats, weight, **kw)
    P = dim * (dim + 1)
    assert got[0].shape == (3,) and got[1].shape == (3, dim, dim + 1) and got[2].shape == (3, P, P)
    for b in range(3):
        one = interpol.ssd_gauss_newton_affine(moving[b], fixed[b], mats[b], weight[b], **kw)
        assert all(close(g[b], o, 1e-13) for g, o in zip(got, one)), b
    # a shared moving image (batch 1) and matrix, the weight and the fixed image carry the batch
    got = interpol.ssd_gauss_newton_affine(moving[:1], fixed, mats[0], weight, **kw)
    assert got[0].shape == (3,)
    for b in range(3):
        one = interpol.ssd_gauss_newton_affine(moving[0], fixed[b], mats[0], weight[b], **kw)
        assert all(close(g[b], o, 1e-13) for g, o in zip(got, one)), b
    # ... and the weight alone
    got = interpol.ssd_gauss_newton_affine(moving[0], fixed[0], mats[0], weight, **kw)
    assert got[0].shape == (3,) and got[2].shape == (3, P, P)
    for b in range(3):
        one = interpol.ssd_gauss_newton_affine(moving[0], fixed[0], mats[0], weight[b], **kw)
        assert all(close(g[b], o, 1e-13) for g, o in zip(got, one)), b


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_a_square_matrix_is_its_first_rows(case):
    inshape, shape = CASES[case]
    dim = len(shape)
    moving, fixed, weight = problem(inshape, shape, 80 + case)
    mat = matrix(dim, scale=0.25)
    full = torch.cat([mat, torch.full((1, dim + 1), 7.0, dtype=mat.dtype)])
    a = interpol.ssd_gauss_newton_affine(moving, fixed, mat, weight, interpolation=2)
    b = interpol.ssd_gauss_newton_affine(moving, fixed, full, weight, interpolation=2)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and b[1].shape == (dim, dim + 1)


def test_validation():
    moving, fixed, weight = problem((5, 4, 6), (4, 5, 3), 90)
    mat = matrix(3)
    f = interpol.ssd_gauss_newton_affine
    with pytest.raises(ValueError, match="floating point"):
        f(moving, fixed.long(), mat)
    with pytest.raises(ValueError, match="floating point"):
        f(moving, fixed, mat.tolist())
    with pytest.raises(ValueError, match="`fixed` must have the dtype and device of `mat`"):
        f(moving, fixed.float(), mat)
    with pytest.raises(ValueError, match="`weight` must have the dtype and device of `mat`"):
        f(moving, fixed, mat, weight.float())
    with pytest.raises(ValueError, match="sets the number of spatial dimensions"):
        f(moving, fixed, mat[:2])                                           # (2, 4): neither D nor D + 1 rows
    with pytest.raises(ValueError, match="sets the number of spatial dimensions"):
        f(moving, fixed, mat[0])
    with pytest.raises(ValueError, match="sets the number of spatial dimensions"):
        f(moving[0, 0], fixed, mat)
    with pytest.raises(ValueError, match="`weight` must have the spatial shape of `fixed`"):
        f(moving, fixed, mat, weight[:3])
    with pytest.raises(ValueError, match="same number of channels"):
        f(moving[:1], fixed, mat)
    with pytest.raises(ValueError, match="[Ii]ncompatible shapes"):
        f(moving.expand(2, *moving.shape), fixed.expand(3, *fixed.shape), mat)
    with torch.enable_grad():
        with pytest.raises(RuntimeError, match="not differentiable"):
            f(moving, fixed, mat.clone().requires_grad_(True))
        with pytest.raises(RuntimeError, match="not differentiable"):
            f(moving.clone().requires_grad_(True), fixed, mat)
    with torch.no_grad():
        assert f(moving, fixed, mat.clone().requires_grad_(True))[2].shape == (12, 12)
    assert "ssd_gauss_newton_affine" in interpol.api.__all__ and interpol.ssd_gauss_newton_affine is f


def test_the_composed_form_serves_four_dimensions_mixed_orders_and_16_bit():
    gen = torch.Generator().manual_seed(5)
    moving, fixed = torch.randn(1, 3, 4, 3, 4, generator=gen, dtype=torch.float64), torch.randn(1, 3, 3, 4, 3, generator=gen, dtype=torch.float64)
    mat = torch.eye(5, dtype=torch.float64)[:4] + 0.0625 * torch.randn(4, 5, generator=gen, dtype=torch.float64)
    kw = dict(interpolation=[1, 2, 3, 1], bound="dct2", extrapolate=True)
    loss, grad, hess = interpol.ssd_gauss_newton_affine(moving, fixed, mat, **kw)
    tl, tg, th = autograd_truth(moving, fixed, mat, None, **kw)
    assert grad.shape == (4, 5) and hess.shape == (20, 20) and close(loss, tl) and close(grad, tg) and close(hess, th)
    m3, f3, w3 = problem((5, 4, 6), (4, 5, 3), 91, dtype=torch.bfloat16)
    got = interpol.ssd_gauss_newton_affine(m3, f3, matrix(3, torch.bfloat16, 0.25), w3, interpolation=1)
    want = interpol.ssd_gauss_newton_affine(m3.double(), f3.double(), matrix(3, torch.float64, 0.25), w3.double(), interpolation=1)
    assert all(g.dtype == torch.bfloat16 for g in got)
    assert all(float((g.double() - w).abs().max()) <= 1e-2 * float(w.abs().max()) for g, w in zip(got, want))


# ---------------------------------------------------------------------------------------------------------------------
# recovery of a known matrix by plain Gauss-Newton
# ---------------------------------------------------------------------------------------------------------------------
TRUE_MAT = [[1.0, 0.0625, -0.03125, 1.5], [-0.0625, 0.96875, 0.03125, -0.75], [0.03125, -0.0625, 1.03125, 2.25]]


def blobs(dtype, device="cpu", seed=7):
    """moving: six Gaussian blobs on 24 x 20 x 22; fixed: its cubic pull through TRUE_MAT on 20 x 22 x 18 (computed in float64)"""
    gen = torch.Generator().manual_seed(seed)
    inshape, shape = (24, 20, 22), (20, 22, 18)
    grid = interpol.identity_grid(inshape, dtype=torch.float64)
    moving = torch.zeros(inshape, dtype=torch.float64)
    for _ in range(6):
        centre = torch.rand(3, generator=gen, dtype=torch.float64) * (torch.tensor(inshape, dtype=torch.float64) - 9) + 4
        width = 2.0 + 2.0 * float(torch.rand(1, generator=gen, dtype=torch.float64))
        moving += (0.5 + float(torch.rand(1, generator=gen, dtype=torch.float64))) * torch.exp(-((grid - centre) ** 2).sum(-1) / (2 * width ** 2))
    moving = moving[None]
    true = torch.tensor(TRUE_MAT, dtype=torch.float64)
    return moving.to(dtype).to(device), true


def recover(moving, true, order, iterations=10):
    """max |mat - true| after each plain Gauss-Newton iteration from the identity; the P x P solve in float64 on the host"""
    dtype, device = moving.dtype, moving.device
    coeff = interpol.spline_coeff_nd(moving.double().cpu(), interpolation=order, bound="dct2", dim=3) if order > 1 else moving.double().cpu()
    kw = dict(interpolation=order, bound="dct2", extrapolate=True)
    fixed = interpol.grid_pull(coeff, interpol.affine_grid(true, (20, 22, 18)), **kw).to(dtype).to(device)
    coeff = coeff.to(dtype).to(device)
    mat = torch.eye(4, dtype=dtype, device=device)[:3]
    errors = []
    for _ in range(iterations):
        loss, g, H = interpol.ssd_gauss_newton_affine(coeff, fixed, mat, **kw)
        step = torch.linalg.solve(H.double().cpu(), g.reshape(-1).double().cpu())
        mat = mat - step.reshape(3, 4).to(dtype).to(device)
        errors.append(float((mat.double().cpu() - true).abs().max()))
    return errors


@pytest.mark.parametrize("order", [1, 3])
def test_recovery_of_a_known_matrix_float64(order):
    errors = recover(*blobs(torch.float64), order)
    print("recovery float64 order %d: max matrix error per iteration %s" % (order, " ".join("%.2g" % e for e in errors)))
    assert errors[-1] <= 1e-8


@pytest.mark.parametrize("order", [1, 2, 3])
def test_recovery_of_a_known_matrix_float32(order):
    errors = recover(*blobs(torch.float32), order)
    print("recovery float32 order %d: max matrix error per iteration %s" % (order, " ".join("%.2g" % e for e in errors)))
    assert errors[-1] <= 1e-4


# ---------------------------------------------------------------------------------------------------------------------
# the truth and the allowance of the device tests (tests/test_ssd_affine_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------
def truth_and_allowance(moving, fixed, mat, weight, tol, **kw):
    """The composed form in float64 on the CPU, fed the upcast operands as `ops` takes them (moving (B|1,C,*in), fixed (B|1,C,*shape),
    mat (B|1,D,D+1), weight None | (B|1,*shape)), and the allowance per entry: the project's bar applied per sample and summed, from
    the reference's own per-sample fields q (= gradient of ssd_gauss_newton) and h (= its Hessian):
        gradient[d, e]: tol sum_o (|q_d| + max|q_d|) |o~_e|;   hessian: tol sum_o (|h_dd'| + max|h_dd'|) |o~_e o~_e'|;
        loss: tol (|ref| + sum_o weight sum_c r_c^2)            (the weights of these tests are non-negative: the sum is 2 ref)"""
    from interpol.codes import pad_codes
    from interpol.autograd import _options
    m, f, a = moving.double().cpu(), fixed.double().cpu(), mat.double().cpu()
    w = None if weight is None else weight.double().cpu()
    dim = a.shape[-1] - 1
    opt = _options(kw.get("bound", "dct2"), kw.get("interpolation", 1), kw.get("extrapolate", True))
    bound, order = pad_codes(opt[0], dim), pad_codes(opt[1], dim)
    want = torch_kernels.ssd_gauss_newton_affine_composed(m, f, a, w, bound, order, int(opt[2]), True)
    shape = list(f.shape[2:])
    o = torch.stack(torch.meshgrid(*[torch.arange(n, dtype=torch.float64) for n in shape], indexing="ij"), -1)
    from interpol.sepgrid import AffineGrid
    lattice = torch.stack([AffineGrid(ab, shape).dense()[0] for ab in a])
    _, q, h = ops.ssd_gauss_newton(m, f, lattice - o, w, bound, order, int(opt[2]), "full")
    B = q.shape[0]
    ot = torch.cat([o, torch.ones_like(o[..., :1])], -1).reshape(-1, dim + 1)
    q, h = q.reshape(B, -1, dim).abs(), h.reshape(B, -1, h.shape[-1]).abs()
    q, h = q + q.amax(1, keepdim=True), h + h.amax(1, keepdim=True)
    ag = tol * torch.einsum("bnd,ne->bde", q, ot)
    kof, k = {}, dim
    for d in range(dim):
        kof[(d, d)] = d
    for d, d2 in itertools.combinations(range(dim), 2):
        kof[(d, d2)] = kof[(d2, d)] = k
        k += 1
    mo = ot[:, :, None] * ot[:, None, :]
    full = torch.stack([torch.stack([h[..., kof[(d, d2)]] for d2 in range(dim)], -1) for d in range(dim)], -2)   # (B, N, D, D)
    P = dim * (dim + 1)
    ah = tol * torch.einsum("bnij,nef->biejf", full, mo).reshape(B, P, P)
    al = tol * 3 * want[0].abs()
    return want, (al, ag, ah)


def worst_ratio(got, want, allow):
    """max over the entries of |got - want| / allowance (0 / 0 counts as 0)"""
    err = (got.double().cpu() - want).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / allow).max())
