"""`interpol.lcc_gauss_newton_affine` on the CPU: the composed form (`torch_kernels.lcc_gauss_newton_affine_composed`) in float64 on
tiny lattices; the helpers that tests/test_lcc_affine_gpu.py shares (`dense_truth`, `truth_and_allowance`).

Truth: `test_lcc_cpu.truth` (the definition restated there, never the function under test) at the dense lattice of the matrix,
contracted here in float64 with the index moments, and autograd through `affine_grid`, `grid_pull` and the window sums of
`test_lcc_cpu.cc_terms` for the gradient.  The lattices are `test_ssd_affine_cpu.CASES`; the thresholds are those of the dense
tests (tests/test_lcc_cpu.py): the gradient to 1e-11 of its largest entry, the Hessian to rtol 1e-11 with atol 1e-13 of its largest
entry, its smallest eigenvalue >= -1e-12 of the largest.

The recovery problem: `test_ssd_affine_cpu.blobs`, fixed = 2 pull(moving, TRUE_MAT) + 5 on 20 x 22 x 18, window 9, twenty plain
Gauss-Newton iterations from the identity.  The positive-part Hessian is conservative, so the convergence is linear: the largest
matrix error starts at 2.25 and was measured at 0.12 (order 1) and 0.10 (order 3) after twenty iterations, with a loss that falls at
every iteration; the bound of 0.25 is twice the measured value.  (Window 5 reaches 0.61 - 0.68 only: not tested to a figure.)
"""
import itertools

import pytest
import torch

import interpol
from interpol import backend, ops
import test_lcc_cpu as lcc
import test_ssd_affine_cpu as aff
import test_ssd_cpu as ssd

CASES, IDS, matrix = aff.CASES, aff.IDS, aff.matrix
WINDOWS = {3: ([3, 9, 5], 3, 5, [1, 5, 3]), 2: ([3, 9], 3, 5, [5, 3]), 1: ([3], 3, 5, [9])}


def dense_truth(moving, fixed, mat, weight, window, eps, hessian=True, **kw):
    """`test_lcc_cpu.truth` in float64 at the dense lattice of the matrices, and its contraction in float64.  moving (B|1,C,*in),
    fixed (B|1,C,*shape), mat (B|1,D,D+1), weight None | (B|1,*shape), of any dtype: widened, the coordinates formed in the dtype of
    `mat`.  The matrices are dyadic (`matrix`): A o + t has no rounding in float64 in any order of the operations, and is asserted
    to be a number of the dtype of `mat`, so it is the coordinate that `AffineGrid` and the kernels form.
    -> ((loss (B), gradient (B,D,D+1), hessian (B,P,P) | None), q (B,N,D), h (B,N,K) | None, ot (N,D+1))"""
    dim = mat.shape[-1] - 1
    shape = list(fixed.shape[2:])
    o = ssd.lattice(shape, mat.dtype).cpu()
    a = mat.cpu().double().reshape([mat.shape[0]] + [1] * dim + [dim, dim + 1])
    x = (a[..., :dim] * o.double().unsqueeze(-2)).sum(-1) + a[..., dim]
    assert torch.equal(x.to(mat.dtype).double(), x)
    disp = (x - o.double()).to(mat.dtype)
    assert torch.equal((o + disp).double(), x)
    w = None if weight is None else weight.cpu()
    loss, q, h, _ = lcc.truth(moving.cpu(), fixed.cpu(), disp, w, window=window, eps=eps, hessian="full" if hessian else None, **kw)
    B = q.shape[0]
    ot = torch.cat([o.double(), torch.ones_like(o[..., :1]).double()], -1).reshape(-1, dim + 1)
    q = q.reshape(B, -1, dim)
    gradient = torch.einsum("bnd,ne->bde", q, ot)
    hess = None
    if hessian:
        h = h.reshape(B, -1, h.shape[-1])
        full = full_blocks(h, dim)
        P = dim * (dim + 1)
        hess = torch.einsum("bnij,ne,nf->biejf", full, ot, ot).reshape(B, P, P)
    return (loss, gradient, hess), q, h, ot


def full_blocks(h, dim):
    """h (B,N,K) in the layout of hessian='full' (the diagonal first, then the upper triangle row by row) -> (B,N,D,D)"""
    kof, k = {}, dim
    for d in range(dim):
        kof[(d, d)] = d
    for d, d2 in itertools.combinations(range(dim), 2):
        kof[(d, d2)] = kof[(d2, d)] = k
        k += 1
    return torch.stack([torch.stack([h[..., kof[(d, d2)]] for d2 in range(dim)], -1) for d in range(dim)], -2)


def truth_and_allowance(moving, fixed, mat, weight, tol, window, eps, **kw):
    """The truth of `dense_truth` and the allowance per entry of `test_ssd_affine_cpu.truth_and_allowance`, built from the truth's
    own per-sample fields: gradient tol sum_o (|q_d| + max|q_d|) |o~_e|, the Hessian likewise with the moments, the loss tol |want|."""
    want, q, h, ot = dense_truth(moving, fixed, mat, weight, window, eps, True, **kw)
    dim = mat.shape[-1] - 1
    B = q.shape[0]
    q, h = q.abs(), h.abs()
    q, h = q + q.amax(1, keepdim=True), h + h.amax(1, keepdim=True)
    ag = tol * torch.einsum("bnd,ne->bde", q, ot.abs())
    P = dim * (dim + 1)
    ah = tol * torch.einsum("bnij,ne,nf->biejf", full_blocks(h, dim), ot.abs(), ot.abs()).reshape(B, P, P)
    al = tol * want[0].abs()
    return want, (al, ag, ah)


def close(got, want, rtol=1e-11, atol=1e-13):
    return bool(((got - want).abs() <= rtol * want.abs() + atol * float(want.abs().max())).all())


# ---------------------------------------------------------------------------------------------------------------------
# 1. gradient and Hessian
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_gradient_is_autograd_of_the_loss(case):
    inshape, shape = CASES[case]
    dim = len(shape)
    worst = 0.0
    for n, (order, bound, extrapolate) in enumerate(itertools.product([1, 2, 3], ["dct2", "dft", "zero"], (False, True))):
        window = WINDOWS[dim][n % 4]
        eps = (1e-5, 1.0)[n % 2]
        moving, fixed, weight = aff.problem(inshape, shape, 100 * case + n, weighted=n % 3 != 0)
        mat = matrix(dim, scale=0.25)
        kw = dict(interpolation=order, bound=bound, extrapolate=extrapolate)
        loss, gradient, none = interpol.lcc_gauss_newton_affine(moving, fixed, mat, weight, window=window, eps=eps, hessian=False, **kw)
        a = mat.clone().requires_grad_()
        I = interpol.grid_pull(moving, interpol.affine_grid(a, shape), **kw)
        wcc = lcc.cc_terms(I[None], fixed[None], None if weight is None else weight[None], lcc.windows(window, dim), eps)[0]
        total = -wcc.sum()
        want, = torch.autograd.grad(total, a)
        assert none is None and loss.shape == () and gradient.shape == (dim, dim + 1) and gradient.dtype == torch.float64
        torch.testing.assert_close(loss, total.detach(), rtol=1e-12, atol=0)
        den = float(want.abs().max())
        worst = max(worst, float((gradient - want).abs().max()) / den)
        assert float((gradient - want).abs().max()) <= 1e-11 * den, (shape, kw, window, eps)
    print("affine gradient against autograd %s -> %s: largest difference / largest entry %.3g" % (inshape, shape, worst))


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_hessian_is_the_dense_hessian_contracted_symmetric_and_positive(case):
    inshape, shape = CASES[case]
    dim = len(shape)
    P = dim * (dim + 1)
    low = 0.0
    for n, (order, bound, extrapolate) in enumerate(((1, "dct2", True), (2, "zero", False), (3, "dft", True), (3, "dst1", False))):
        moving, fixed, weight = aff.problem(inshape, shape, 700 + 10 * case + n, weighted=n % 2 == 0)
        mat = matrix(dim, scale=0.25)
        kw = dict(interpolation=order, bound=bound, extrapolate=extrapolate)
        window = WINDOWS[dim][n % 2]
        want = dense_truth(moving[None], fixed[None], mat[None], None if weight is None else weight[None], window, 1e-3, **kw)[0]
        loss, gradient, hess = interpol.lcc_gauss_newton_affine(moving, fixed, mat, weight, window=window, eps=1e-3, **kw)
        assert loss.shape == () and gradient.shape == (dim, dim + 1) and hess.shape == (P, P)
        torch.testing.assert_close(loss, want[0][0], rtol=1e-12, atol=0)
        assert close(gradient, want[1][0]) and close(hess, want[2][0])
        assert torch.equal(hess, hess.mT)
        ev = torch.linalg.eigvalsh(hess)
        low = min(low, float(ev[0]) / max(float(ev[-1]), 1e-300))
        assert float(ev[0]) >= -1e-12 * float(ev[-1])
        l0, g0, none = interpol.lcc_gauss_newton_affine(moving, fixed, mat, weight, window=window, eps=1e-3, hessian=False, **kw)
        assert none is None and torch.equal(l0, loss) and torch.equal(g0, gradient)
    print("affine hessian %s: smallest eigenvalue / largest %.3g" % (shape, low))


# ---------------------------------------------------------------------------------------------------------------------
# 2. batch and options
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_a_batch_of_matrices_is_one_call_per_matrix(case):
    inshape, shape = CASES[case]
    dim = len(shape)
    moving, fixed, weight = aff.problem(inshape, shape, 70 + case, B=3)
    mats = torch.stack([matrix(dim, scale=s) for s in (0.25, 0.5, -0.125)])
    mats[1, 0, 0] += 0.0625
    kw = dict(interpolation=3, bound="dct2", extrapolate=False, window=3, eps=1e-3)
    got = interpol.lcc_gauss_newton_affine(moving, fixed, mats, weight, **kw)
    P = dim * (dim + 1)
    assert got[0].shape == (3,) and got[1].shape == (3, dim, dim + 1) and got[2].shape == (3, P, P)
    for b in range(3):
        one = interpol.lcc_gauss_newton_affine(moving[b], fixed[b], mats[b], weight[b], **kw)
        assert all(aff.close(g[b], o, 1e-13) for g, o in zip(got, one)), b
    # a shared moving image (batch 1) and matrix, the weight and the fixed image carry the batch
    got = interpol.lcc_gauss_newton_affine(moving[:1], fixed, mats[0], weight, **kw)
    assert got[0].shape == (3,)
    for b in range(3):
        one = interpol.lcc_gauss_newton_affine(moving[0], fixed[b], mats[0], weight[b], **kw)
        assert all(aff.close(g[b], o, 1e-13) for g, o in zip(got, one)), b


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_a_square_matrix_is_its_first_rows(case):
    inshape, shape = CASES[case]
    dim = len(shape)
    moving, fixed, weight = aff.problem(inshape, shape, 80 + case)
    mat = matrix(dim, scale=0.25)
    full = torch.cat([mat, torch.full((1, dim + 1), 7.0, dtype=mat.dtype)])
    a = interpol.lcc_gauss_newton_affine(moving, fixed, mat, weight, window=3, interpolation=2)
    b = interpol.lcc_gauss_newton_affine(moving, fixed, full, weight, window=3, interpolation=2)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and b[1].shape == (dim, dim + 1)


def test_weight_scales_the_three_outputs():
    """a constant weight k multiplies loss, gradient and Hessian by k; None is a weight of one"""
    moving, fixed, weight = aff.problem((7, 4), (6, 5), 910)
    mat = matrix(2, scale=0.25)
    kw = dict(interpolation=3, bound="replicate", extrapolate=True, window=5, eps=1e-3)
    one = interpol.lcc_gauss_newton_affine(moving, fixed, mat, None, **kw)
    ones = interpol.lcc_gauss_newton_affine(moving, fixed, mat, torch.ones_like(weight), **kw)
    assert all(torch.equal(a, b) for a, b in zip(one, ones))
    three = interpol.lcc_gauss_newton_affine(moving, fixed, mat, torch.full_like(weight, 3.0), **kw)
    for a, b in zip(one, three):
        torch.testing.assert_close(3 * a, b, rtol=1e-12, atol=1e-13 * float(b.abs().max()))


def test_prefilter_is_spline_coeff_nd_first():
    moving, fixed, weight = aff.problem((5, 4, 6), (4, 5, 3), 920)
    mat = matrix(3, scale=0.25)
    for order in (1, 3, [1, 2, 3]):
        kw = dict(interpolation=order, bound="dct2", extrapolate=True, window=3)
        got = interpol.lcc_gauss_newton_affine(moving, fixed, mat, weight, prefilter=True, **kw)
        coeff = interpol.spline_coeff_nd(moving, interpolation=order, bound="dct2", dim=3)
        want = interpol.lcc_gauss_newton_affine(coeff, fixed, mat, weight, **kw)
        plain = interpol.lcc_gauss_newton_affine(moving, fixed, mat, weight, **kw)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
        assert torch.equal(got[1], plain[1]) == (order == 1)


def test_loss_is_invariant_under_an_affine_change_of_fixed():
    """fixed -> 2 fixed + 5, as tests/test_lcc_cpu.py states it: eps = 1e-12, tolerance 1e-8 relative"""
    worst = 0.0
    for case, (inshape, shape) in enumerate(CASES):
        moving, fixed, weight = aff.problem(inshape, shape, 800 + case)
        kw = dict(interpolation=1, bound="dct2", extrapolate=True, window=5, eps=1e-12, hessian=False)
        mat = matrix(len(shape), scale=0.25)
        base = interpol.lcc_gauss_newton_affine(moving, fixed, mat, weight, **kw)[0]
        got = interpol.lcc_gauss_newton_affine(moving, 2.0 * fixed + 5.0, mat, weight, **kw)[0]
        worst = max(worst, float(((got - base) / base).abs()))
    print("affine invariance: largest relative change of the loss %.3g" % worst)
    assert worst <= 1e-8


# ---------------------------------------------------------------------------------------------------------------------
# 3. arguments
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    moving, fixed, weight = aff.problem((5, 4, 6), (4, 5, 3), 950)
    mat = matrix(3)
    f = interpol.lcc_gauss_newton_affine
    for bad in (4, 0, -3, [3, 2, 5], 3.0, True, [3, 5], [3, 5, 7, 9], []):
        with pytest.raises(ValueError, match="window"):
            f(moving, fixed, mat, weight, window=bad)
    for bad in (0, 0.0, -1e-5, float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="eps"):
            f(moving, fixed, mat, weight, eps=bad)
    with pytest.raises(ValueError, match="floating point"):
        f(moving, fixed.long(), mat)
    with pytest.raises(ValueError, match="`fixed` must have the dtype and device of `mat`"):
        f(moving, fixed.float(), mat)
    with pytest.raises(ValueError, match="`weight` must have the dtype and device of `mat`"):
        f(moving, fixed, mat, weight.float())
    with pytest.raises(ValueError, match="dtype and device"):
        f(moving, fixed.to("meta"), mat)
    with pytest.raises(ValueError, match="sets the number of spatial dimensions"):
        f(moving, fixed, mat[:2])                                           # (2, 4): neither D nor D + 1 rows
    with pytest.raises(ValueError, match="sets the number of spatial dimensions"):
        f(moving, fixed, mat[0])
    with pytest.raises(ValueError, match="`weight` must have the spatial shape of `fixed`"):
        f(moving, fixed, mat, weight[:3])
    with pytest.raises(ValueError, match="same number of channels"):
        f(moving[:1], fixed, mat)
    with torch.enable_grad():
        with pytest.raises(RuntimeError, match="not differentiable"):
            f(moving, fixed, mat.clone().requires_grad_(True))
        with pytest.raises(RuntimeError, match="not differentiable"):
            f(moving.clone().requires_grad_(True), fixed, mat)
    with torch.no_grad():
        assert f(moving, fixed, mat.clone().requires_grad_(True), window=3)[2].shape == (12, 12)
    backend.jitfields = True
    try:
        with pytest.raises(RuntimeError, match="jitfields"):
            f(moving, fixed, mat, weight)
    finally:
        backend.jitfields = False
    assert "lcc_gauss_newton_affine" in interpol.api.__all__ and interpol.lcc_gauss_newton_affine is f


def test_the_composed_form_serves_four_dimensions_mixed_orders_16_bit_and_window_11():
    gen = torch.Generator().manual_seed(5)
    moving, fixed = torch.randn(1, 3, 4, 3, 4, generator=gen, dtype=torch.float64), torch.randn(1, 3, 3, 4, 3, generator=gen, dtype=torch.float64)
    mat = torch.eye(5, dtype=torch.float64)[:4] + 0.0625 * torch.randn(4, 5, generator=gen, dtype=torch.float64)
    kw = dict(interpolation=[1, 2, 3, 1], bound="dct2", extrapolate=True)
    window = [3, 1, 5, 3]
    loss, grad, hess = interpol.lcc_gauss_newton_affine(moving, fixed, mat, window=window, eps=1e-3, **kw)
    assert loss.shape == () and grad.shape == (4, 5) and hess.shape == (20, 20) and torch.equal(hess, hess.mT)
    a = mat.clone().requires_grad_()
    I = interpol.grid_pull(moving, interpol.affine_grid(a, list(fixed.shape[1:])), **kw)
    total = -lcc.cc_terms(I[None], fixed[None], None, window, 1e-3)[0].sum()
    want, = torch.autograd.grad(total, a)
    torch.testing.assert_close(loss, total.detach(), rtol=1e-12, atol=0)
    assert float((grad - want).abs().max()) <= 1e-11 * float(want.abs().max())
    # window 11 on a 3-D lattice, mixed orders
    m3, f3, w3 = aff.problem((5, 4, 6), (4, 5, 3), 91)
    for kw3 in (dict(window=11, interpolation=1), dict(window=3, interpolation=[1, 2, 3])):
        got = interpol.lcc_gauss_newton_affine(m3, f3, matrix(3, scale=0.25), w3, eps=1e-3, **kw3)
        want = dense_truth(m3[None], f3[None], matrix(3, scale=0.25)[None], w3[None], kw3["window"], 1e-3,
                           interpolation=kw3["interpolation"], bound="dct2", extrapolate=True)[0]
        assert close(got[1], want[1][0]) and close(got[2], want[2][0])
    # 16-bit storage computes in float32 and is rounded once
    mb, fb, wb = aff.problem((5, 4, 6), (4, 5, 3), 91, dtype=torch.bfloat16)
    got = interpol.lcc_gauss_newton_affine(mb, fb, matrix(3, torch.bfloat16, 0.25), wb, window=3, eps=1e-2)
    ref = interpol.lcc_gauss_newton_affine(mb.float(), fb.float(), matrix(3, torch.float32, 0.25), wb.float(), window=3, eps=1e-2)
    assert all(g.dtype == torch.bfloat16 and torch.equal(g, r.to(torch.bfloat16)) for g, r in zip(got, ref))


def test_the_kernel_table_is_reached_with_folded_operands(monkeypatch):
    moving, fixed, weight = aff.problem((5, 4, 6), (4, 5, 3), 960, B=2)
    seen = []
    fn = ops.lcc_gauss_newton_affine

    def spy(m, f, a, w, *rest):
        seen.append((m, f, a, w, rest))
        return fn(m, f, a, w, *rest)

    monkeypatch.setattr(ops, "lcc_gauss_newton_affine", spy)
    interpol.lcc_gauss_newton_affine(moving, fixed[0], matrix(3), weight, window=[3, 5, 1], eps=0.5, hessian=False)
    m, f, a, w, rest = seen[-1]
    assert m.shape[0] == 2 and f.shape[0] == 1 and a.shape == (1, 3, 4) and w.shape[0] == 2 and f.data_ptr() == fixed.data_ptr()
    assert rest[-3:] == (False, [3, 5, 1], 0.5)


# ---------------------------------------------------------------------------------------------------------------------
# 4. recovery of a known matrix by plain Gauss-Newton under an intensity change
# ---------------------------------------------------------------------------------------------------------------------
def recover(moving, true, order, window=9, iterations=20):
    """(losses, max |mat - true| after each iteration) of plain Gauss-Newton from the identity; fixed = 2 pull(moving, true) + 5; the
    P x P solve in float64 on the host"""
    dtype, device = moving.dtype, moving.device
    coeff = interpol.spline_coeff_nd(moving.double().cpu(), interpolation=order, bound="dct2", dim=3) if order > 1 else moving.double().cpu()
    kw = dict(interpolation=order, bound="dct2", extrapolate=True)
    fixed = (2 * interpol.grid_pull(coeff, interpol.affine_grid(true, (20, 22, 18)), **kw) + 5).to(dtype).to(device)
    coeff = coeff.to(dtype).to(device)
    mat = torch.eye(4, dtype=dtype, device=device)[:3]
    losses, errors = [], []
    for _ in range(iterations):
        loss, g, H = interpol.lcc_gauss_newton_affine(coeff, fixed, mat, window=window, **kw)
        step = torch.linalg.solve(H.double().cpu(), g.reshape(-1).double().cpu())
        mat = mat - step.reshape(3, 4).to(dtype).to(device)
        losses.append(float(loss))
        errors.append(float((mat.double().cpu() - true).abs().max()))
    return losses, errors


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("order", [1, 3])
def test_recovery_of_a_known_matrix(order, dtype):
    losses, errors = recover(*aff.blobs(dtype), order)
    print("lcc affine recovery %s order %d: max matrix error per iteration %s" % (dtype, order, " ".join("%.2g" % e for e in errors)))
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    assert errors[-1] <= 0.25
