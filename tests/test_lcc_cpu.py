"""`interpol.lcc_gauss_newton` on the CPU: the composed form (interpol/torch_kernels.py: lcc_gauss_newton_composed).

Truth: the definition restated below (`truth`) in float64 -- `grid_pull` / `grid_grad` at a displacement, window sums written here
as explicit loops over the shifts, the second moments in their central form (the same numbers as S_II - S_I^2 / n, S_JJ - S_J^2 / n
and S_IJ - S_I S_J / n, without the cancellation), the closed-form gradient -- and autograd through `grid_pull` plus those window sums for the
gradient; never the function under test.

The device test (tests/test_lcc_gpu.py) shares `problem`, `truth`, `item_ratio` and the helpers of tests/test_ssd_cpu.py
(`lattice`, `nudged`, `in_view`, `ratio`).

Measured on the CPU in float64: the gradient against autograd differs by at most 5.1e-12 of its largest entry (1-D, window 3,
eps 1e-5: the plain second moments of the composed form against the central ones here; 5e-13 in 2-D and 3-D; the figure per shape
is printed); the smallest eigenvalue of the assembled Hessians is >= -1.4e-16 of the largest; the loss under affine changes
of both images (eps = 1e-12) moves by at most 2.8e-10 relative.
"""
import itertools

import pytest
import torch

import interpol
from interpol import ops
import test_ssd_cpu as ssd
import test_regulariser_solve_cpu as st

BOUNDS = ssd.BOUNDS
ORDERS = [1, 2, 3]
CPU_SHAPES = [((11,), (9,)), ((9, 12), (8, 13)), ((5, 6, 7), (4, 6, 5)), ((1, 2, 3), (2, 1, 3))]
IDS = ssd.IDS


def problem(inshape, shape, seed, dtype=torch.float64, C=2, B=2, sigma=2.0, weighted=True, offset=0.0):
    """moving (B, C, *inshape) ~ N(0, 1) + offset; fixed (C, *shape) -- no batch -- = 0.8 (moving[0] pulled linearly at the lattice
    of `fixed` stretched onto `inshape` plus 0.5 N(0, 1) displacements) + 0.3 N(0, 1) + offset; disp (B, *shape, D) = sigma N(0, 1);
    weight (B, *shape) in [0.5, 1.5) or None.  Drawn in float64 and rounded to `dtype` once."""
    gen = torch.Generator().manual_seed(seed)
    dim = len(shape)
    rnd = lambda *s: torch.randn(list(s), generator=gen, dtype=torch.float64)
    moving = rnd(B, C, *inshape) + offset
    stretch = torch.tensor([(a - 1) / (b - 1) if b > 1 else 0.0 for a, b in zip(inshape, shape)], dtype=torch.float64)
    at = ssd.lattice(shape, torch.float64) * stretch + 0.5 * rnd(*shape, dim)
    fixed = 0.8 * interpol.grid_pull(moving[0], at, interpolation=1, bound="dct2", extrapolate=True) + 0.3 * rnd(C, *shape) + offset
    disp = sigma * rnd(B, *shape, dim)
    weight = 0.5 + torch.rand([B, *shape], generator=gen, dtype=torch.float64)
    return moving.to(dtype), fixed.to(dtype), disp.to(dtype), (weight.to(dtype) if weighted else None)


def windows(window, dim):
    return list(window)[:dim] if isinstance(window, (list, tuple)) else [window] * dim


def box(x, window):
    """the zero-padded window sum over the last len(window) dims, one explicit loop over the shifts per dim"""
    dim = len(window)
    for d, w in enumerate(window):
        r = (w - 1) // 2
        axis = x.dim() - dim + d
        n = x.shape[axis]
        out = torch.zeros_like(x)
        for t in range(-r, r + 1):
            lo, hi = max(0, -t), min(n, n - t)                           # out[o] += x[o + t] for o + t inside
            if hi > lo:
                out.narrow(axis, lo, hi - lo).add_(x.narrow(axis, lo + t, hi - lo))
        x = out
    return x


CENTRAL_UP_TO = 27                                                   # offsets of a window (clipped to the extents)


def central_moments(I, J, window, n):
    """(vI, vJ, cross) = S_II - S_I^2 / n, S_JJ - S_J^2 / n, S_IJ - S_I S_J / n.  Where the window has at most CENTRAL_UP_TO offsets
    (|t_d| <= min(r_d, extent_d - 1)) they are summed in their central form, sum (I - mean_I)(J - mean_J) with the means of the
    window, one term per offset: the same numbers without the cancellation.  With three nearly equal points in a window the rounding
    of S_II, divided by a den that falls to eps = 1e-5, is 0.46 of the float64 bar on its own (measured against a long-double
    evaluation; the central form is within 0.004).  Larger windows hold eight points or more even where the edges clip them, a
    variance below 1e-3 is then out of reach of N(0, 1) draws (p < 1e-10), and the plain form loses log2(1 + offset^2) < 7 bits."""
    dim = len(window)
    r = [min((w - 1) // 2, nd - 1) for w, nd in zip(window, I.shape[-dim:])]
    offsets = list(itertools.product(*[range(2 * rd + 1) for rd in r]))
    SI, SJ = box(I, window), box(J, window)
    if len(offsets) > CENTRAL_UP_TO:
        return ((box(I * I, window) - SI * SI / n).clamp_min(0), (box(J * J, window) - SJ * SJ / n).clamp_min(0),
                box(I * J, window) - SI * SJ / n)
    mI, mJ = SI / n, SJ / n
    pad = [q for rd in reversed(r) for q in (rd, rd)]
    Ip, Jp = torch.nn.functional.pad(I, pad), torch.nn.functional.pad(J, pad)
    inside = torch.nn.functional.pad(torch.ones(I.shape[-dim:], dtype=I.dtype), pad)
    vI, vJ, cross = torch.zeros_like(mI + mJ), torch.zeros_like(mI + mJ), torch.zeros_like(mI + mJ)
    for t in offsets:
        cut = lambda x: x[(..., *[slice(td, td + nd) for td, nd in zip(t, I.shape[-dim:])])]
        m = cut(inside)
        dI, dJ = m * (cut(Ip) - mI), m * (cut(Jp) - mJ)
        vI, vJ, cross = vI + dI * dI, vJ + dJ * dJ, cross + dI * dJ
    return vI, vJ, cross


def cc_terms(I, J, weight, window, eps):
    """(weight cc, cross, vJ, den, n, S_I, S_J, weight) of the definition; I, J (B|1, C, *shape), weight None or (B|1, *shape)"""
    n = box(torch.ones(I.shape[2:], dtype=I.dtype), window)
    SI, SJ = box(I, window), box(J, window)
    vI, vJ, cross = central_moments(I, J, window, n)
    den = vI * vJ + eps
    wt = 1.0 if weight is None else weight.unsqueeze(1)
    return wt * cross * cross / den, cross, vJ, den, n, SI, SJ, wt


def truth(moving, fixed, disp, weight, window=9, eps=1e-5, hessian="full", **kw):
    """The definition in float64 on the inputs as given (widened), at the coordinates o + disp formed in the dtype of `disp` and then
    widened.  fixed (C, *shape) or (B, C, *shape).  -> (loss (B), gradient, hessian, mean cc)"""
    dim = disp.shape[-1]
    window = windows(window, dim)
    o = ssd.lattice(disp.shape[-dim - 1:-1], disp.dtype)
    x = (o + disp).double()
    d64 = x - o.double()
    assert torch.equal(o.double() + d64, x)
    m, J = moving.double(), fixed.double()
    if J.dim() == dim + 1:
        J = J[None]
    w = None if weight is None else weight.double()
    I = interpol.grid_pull(m, d64, displacement=True, **kw)
    G = interpol.grid_grad(m, d64, displacement=True, **kw)
    wcc, cross, vJ, den, n, SI, SJ, wt = cc_terms(I, J, w, window, eps)
    a = wt * 2 * cross / den
    c = wt * 2 * cross * cross * vJ / (den * den)
    f = (a * SJ - c * SI) / n
    A, C, F = box(a, window), box(c, window), box(f, window)
    dI = -J * A + I * C + F
    loss = -wcc.flatten(1).sum(1)
    gradient = (dI.unsqueeze(-1) * G).sum(1)
    pairs = [(d, d) for d in range(dim)]
    if hessian == "full":
        pairs += [(d, e) for d in range(dim) for e in range(d + 1, dim)]
    hess = None if hessian is None else torch.stack([(C * G[..., d] * G[..., e]).sum(1) for d, e in pairs], -1)
    return loss, gradient, hess, float((wcc / wt).mean())


def item_ratio(got, want, tol, with_scale=True):
    """max over the items of max |got - want| / (tol |want| + tol scale), scale = max |want| over the item (0 for the loss)"""
    got, want = got.detach().cpu().double(), want.double()
    worst = 0.0
    for b in range(want.shape[0]):
        scale = float(want[b].abs().max()) if with_scale else 0.0
        worst = max(worst, ssd.ratio(got[b], want[b], tol, scale))
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# 1. the gradient is d loss / d disp
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(CPU_SHAPES)), ids=IDS(CPU_SHAPES))
def test_gradient_is_autograd_of_the_loss(case):
    inshape, shape = CPU_SHAPES[case]
    dim = len(shape)
    worst = 0.0
    for n, (order, bound, extrapolate) in enumerate(itertools.product(ORDERS, BOUNDS, (False, True))):
        window = ([3, 9, 5][:dim], 3, 5, [1, 5, 3][-dim:])[n % 4]
        eps = (1e-5, 1.0)[n % 2]
        moving, fixed, disp, weight = problem(inshape, shape, 100 * case + n, weighted=n % 3 != 0, sigma=(2.0, 0.4)[n % 2],
                                              offset=(0.0, 10.0)[(n // 2) % 2] if eps == 1.0 else 0.0)
        kw = dict(interpolation=order, bound=bound, extrapolate=extrapolate)
        loss, gradient, _ = interpol.lcc_gauss_newton(moving, fixed, disp, weight, window=window, eps=eps, hessian=None, **kw)
        u = disp.clone().requires_grad_()
        I = interpol.grid_pull(moving, u, displacement=True, **kw)
        wcc = cc_terms(I, fixed[None], weight, windows(window, dim), eps)[0]
        total = -wcc.sum()
        want, = torch.autograd.grad(total, u)
        assert loss.shape == (2,) and gradient.shape == disp.shape and gradient.dtype == torch.float64
        torch.testing.assert_close(loss.sum(), total.detach(), rtol=1e-12, atol=0)
        den = float(want.abs().max())
        if den:
            worst = max(worst, float((gradient - want).abs().max()) / den)
            assert float((gradient - want).abs().max()) <= 1e-11 * den, (shape, kw, window, eps)
    print("gradient against autograd %s -> %s: largest difference / largest entry %.3g" % (inshape, shape, worst))


# ---------------------------------------------------------------------------------------------------------------------
# 2. the Hessian, the bounds of the loss, the invariance
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(CPU_SHAPES)), ids=IDS(CPU_SHAPES))
def test_hessian_is_the_weighted_sum_of_outer_products_and_positive(case):
    inshape, shape = CPU_SHAPES[case]
    dim = len(shape)
    low = 0.0
    for n, (order, bound, extrapolate) in enumerate(((1, "dct2", True), (2, "zero", False), (3, "dft", True), (3, "dst1", False))):
        moving, fixed, disp, weight = problem(inshape, shape, 700 + 10 * case + n, weighted=n % 2 == 0, sigma=0.7)
        kw = dict(interpolation=order, bound=bound, extrapolate=extrapolate)
        window = (3, [3, 9, 5][:dim])[n % 2]
        want = truth(moving, fixed, disp, weight, window=window, eps=1e-3, **kw)
        loss, gradient, full = interpol.lcc_gauss_newton(moving, fixed, disp, weight, window=window, eps=1e-3, **kw)
        assert full.shape == (2, *shape, dim * (dim + 1) // 2)
        torch.testing.assert_close(full, want[2], rtol=1e-11, atol=1e-13 * float(want[2].abs().max()))
        torch.testing.assert_close(gradient, want[1], rtol=1e-11, atol=1e-13 * float(want[1].abs().max()))
        torch.testing.assert_close(loss, want[0], rtol=1e-12, atol=0)
        l1, g1, diag = interpol.lcc_gauss_newton(moving, fixed, disp, weight, window=window, eps=1e-3, hessian="diagonal", **kw)
        assert diag.shape == (2, *shape, dim) and torch.equal(diag, full[..., :dim])
        l0, g0, none = interpol.lcc_gauss_newton(moving, fixed, disp, weight, window=window, eps=1e-3, hessian=None, **kw)
        assert none is None
        for l, g in ((l1, g1), (l0, g0)):
            assert torch.equal(l, loss) and torch.equal(g, gradient)
        ev = torch.linalg.eigvalsh(st.unpack(full, dim))
        low = min(low, float(ev.min()) / max(float(ev.max()), 1e-300))
        assert float(ev.min()) >= -1e-12 * float(ev.max())
        # Cauchy-Schwarz: 0 <= cc <= 1 per channel and voxel
        C = moving.shape[1]
        wsum = (weight.flatten(1).sum(1) if weight is not None else torch.full([2], float(disp[0].numel() // dim), dtype=torch.float64))
        assert bool((loss <= 0).all()) and bool((loss >= -C * wsum).all())
    print("hessian %s: smallest eigenvalue / largest %.3g" % (shape, low))


def test_loss_is_invariant_under_affine_changes_of_both_images():
    """cc is a ratio of second central moments: alpha and alpha' cancel, beta and beta' drop out.  What is left: eps against
    vI vJ (1e-12 against products of sums of >= 2 squared N(0, 1) draws: below 1e-9 at these seeds) and the rounding of the moments,
    amplified by (mean / spread)^2 <= 100 times 2^-52.  Tolerance 1e-8 relative; measured 2.8e-10."""
    worst = 0.0
    for case, (inshape, shape) in enumerate(CPU_SHAPES[:3]):
        moving, fixed, disp, weight = problem(inshape, shape, 800 + case, sigma=0.7)
        kw = dict(interpolation=1, bound="dct2", extrapolate=True, window=5, eps=1e-12, hessian=None)
        base = interpol.lcc_gauss_newton(moving, fixed, disp, weight, **kw)[0]
        for alpha, beta, alpha2, beta2 in ((2.0, 5.0, 1.0, 0.0), (1.0, 0.0, -0.5, 3.0), (-3.0, -2.0, 0.25, 7.0)):
            got = interpol.lcc_gauss_newton(alpha2 * moving + beta2, alpha * fixed + beta, disp, weight, **kw)[0]
            worst = max(worst, float(((got - base) / base).abs().max()))
    print("invariance: largest relative change of the loss %.3g" % worst)
    assert worst <= 1e-8


# ---------------------------------------------------------------------------------------------------------------------
# 3. one Gauss-Newton step lowers the objective where the sum of squares cannot
# ---------------------------------------------------------------------------------------------------------------------
def gauss_newton_step(moving, fixed, disp, membrane=0.01, window=5):
    """-> (objective before, objective after) of one step disp - (H + L)^-1 (g + L disp)"""
    kw = dict(interpolation=3, bound="dct2", extrapolate=True, window=window, eps=1e-8)
    reg = dict(membrane=membrane, bound="dct2")
    loss, g, h = interpol.lcc_gauss_newton(moving, fixed, disp, hessian="full", **kw)
    before = loss + interpol.regulariser_energy(disp, **reg)
    x = interpol.regulariser_solve(g + interpol.regulariser(disp, **reg), h, max_iter=16, **reg)
    new = disp - x
    after = interpol.lcc_gauss_newton(moving, fixed, new, hessian=None, **kw)[0] + interpol.regulariser_energy(new, **reg)
    return before, after


def rescaled_blobs(n, dim, dtype, device="cpu"):
    moving, fixed = ssd.blobs(n, dim, dtype, device)
    return moving, 2 * fixed + 5


def test_one_gauss_newton_step_lowers_the_objective():
    moving, fixed = rescaled_blobs(16, 2, torch.float64)
    disp = torch.zeros(16, 16, 2, dtype=torch.float64)
    before, after = gauss_newton_step(moving, fixed, disp)
    print("lcc objective %.6g -> %.6g" % (float(before), float(after)))
    assert float(after) < float(before) < 0
    # the sum of squares sees the intensity change, not the shift: its step does not bring the images together
    sb, sa = ssd.gauss_newton_step(moving, fixed, disp)
    assert float(sa) > 0.9 * float(sb)


# ---------------------------------------------------------------------------------------------------------------------
# 4. arguments
# ---------------------------------------------------------------------------------------------------------------------
def test_batch_broadcasting_copies_nothing(monkeypatch):
    inshape, shape = (4, 5, 6), (3, 5, 4)
    moving, fixed, disp, weight = problem(inshape, shape, 900, C=3)
    kw = dict(interpolation=2, bound="dct1", extrapolate=False, window=3)
    seen = []
    fn = ops.lcc_gauss_newton

    def spy(m, f, u, w, *a):
        seen.append((m, f, u, w))
        return fn(m, f, u, w, *a)

    monkeypatch.setattr(ops, "lcc_gauss_newton", spy)
    loss, g, h = interpol.lcc_gauss_newton(moving, fixed, disp, weight, **kw)                    # fixed without a batch
    m, f, u, w = seen[-1]
    assert f.shape == (1, 3, *shape) and f.data_ptr() == fixed.data_ptr() and m.data_ptr() == moving.data_ptr()
    assert u.data_ptr() == disp.data_ptr() and w.data_ptr() == weight.data_ptr()
    le, ge, he = interpol.lcc_gauss_newton(moving, fixed.expand(2, *fixed.shape).contiguous(), disp, weight, **kw)
    assert torch.equal(loss, le) and torch.equal(g, ge) and torch.equal(h, he)
    ls, gs, hs = interpol.lcc_gauss_newton(moving, fixed[None].expand(2, *fixed.shape), disp, weight[:1].expand_as(weight), **kw)
    m, f, u, w = seen[-1]
    assert f.stride(0) == 0 and f.data_ptr() == fixed.data_ptr() and w.stride(0) == 0 and w.data_ptr() == weight.data_ptr()
    # only `moving` has a batch: the others serve every item
    l2, g2, h2 = interpol.lcc_gauss_newton(moving, fixed, disp[0], weight[0], **kw)
    m, f, u, w = seen[-1]
    assert u.shape[0] == 1 and w.shape[0] == 1 and u.data_ptr() == disp.data_ptr()
    assert l2.shape == (2,) and g2.shape == disp.shape and h2.shape == h.shape
    assert torch.equal(l2[0], loss[0]) and torch.equal(g2[0], g[0]) and torch.equal(h2[0], h[0])
    # leading batch dimensions fold; no batch at all gives a scalar loss
    l3, g3, h3 = interpol.lcc_gauss_newton(moving.reshape(2, 1, *moving.shape[1:]), fixed, disp.reshape(2, 1, *disp.shape[1:]),
                                           weight, **kw)
    assert l3.shape == (2, 2) and g3.shape == (2, 2, *shape, 3) and h3.shape == (2, 2, *shape, 6)
    assert torch.equal(l3[0, 0], loss[0]) and torch.equal(g3[1, 1], g[1])
    l4, g4, h4 = interpol.lcc_gauss_newton(moving[0], fixed, disp[0], weight[0], **kw)
    assert l4.shape == () and g4.shape == disp[0].shape and torch.equal(g4, g[0]) and torch.equal(l4, loss[0])
    # only `weight` has a batch
    for kind in ("full", "diagonal", None):
        l5, g5, h5 = interpol.lcc_gauss_newton(moving[0], fixed, disp[0], weight, hessian=kind, **kw)
        assert l5.shape == (2,) and g5.shape == disp.shape and (h5 is None) == (kind is None)
        for b in range(2):
            lb, gb, hb = interpol.lcc_gauss_newton(moving[0], fixed, disp[0], weight[b], hessian=kind, **kw)
            assert torch.equal(l5[b], lb) and torch.equal(g5[b], gb) and (kind is None or torch.equal(h5[b], hb))


def test_weight_scales_the_three_outputs():
    """a constant weight k multiplies loss, gradient and Hessian by k; None is a weight of one"""
    moving, fixed, disp, weight = problem((9, 12), (8, 13), 910)
    kw = dict(interpolation=3, bound="replicate", extrapolate=True, window=5, eps=1e-3)
    one = interpol.lcc_gauss_newton(moving, fixed, disp, None, **kw)
    ones = interpol.lcc_gauss_newton(moving, fixed, disp, torch.ones_like(weight), **kw)
    assert all(torch.equal(a, b) for a, b in zip(one, ones))
    three = interpol.lcc_gauss_newton(moving, fixed, disp, torch.full_like(weight, 3.0), **kw)
    for a, b in zip(one, three):
        torch.testing.assert_close(3 * a, b, rtol=1e-12, atol=1e-13 * float(b.abs().max()))
    # a weight that varies enters as the definition says
    want = truth(moving, fixed, disp, weight, **kw)
    got = interpol.lcc_gauss_newton(moving, fixed, disp, weight, **kw)
    for a, b in zip(got, want[:3]):
        torch.testing.assert_close(a, b, rtol=1e-11, atol=1e-13 * float(b.abs().max()))


def test_prefilter_is_spline_coeff_nd_first():
    moving, fixed, disp, weight = problem((5, 6, 7), (4, 6, 5), 920)
    for order in (1, 3, [1, 2, 3]):
        kw = dict(interpolation=order, bound="dct2", extrapolate=True, window=3)
        got = interpol.lcc_gauss_newton(moving, fixed, disp, weight, prefilter=True, **kw)
        coeff = interpol.spline_coeff_nd(moving, interpolation=order, bound="dct2", dim=3)
        want = interpol.lcc_gauss_newton(coeff, fixed, disp, weight, **kw)
        plain = interpol.lcc_gauss_newton(moving, fixed, disp, weight, **kw)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
        assert torch.equal(got[1], plain[1]) == (order == 1)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_sixteen_bit_inputs_compute_in_float32_and_round_once(dtype):
    moving, fixed, disp, weight = problem((5, 6, 7), (4, 6, 5), 930, dtype=dtype, sigma=0.7)
    kw = dict(interpolation=3, bound="dct2", extrapolate=True, window=3, eps=1e-2)
    got = interpol.lcc_gauss_newton(moving, fixed, disp, weight, **kw)
    want = interpol.lcc_gauss_newton(moving.float(), fixed.float(), disp.float(), weight.float(), **kw)
    for a, b in zip(got, want):
        assert a.dtype == dtype and b.dtype == torch.float32 and torch.equal(a, b.to(dtype))


def test_four_dimensions_and_aliases():
    inshape, shape = (3, 2, 4, 3), (2, 3, 3, 2)
    moving, fixed, disp, weight = problem(inshape, shape, 940, C=2, sigma=0.8)
    kw = dict(interpolation=["linear", 2, "cubic", 1], bound=["mirror", "dct2", "circular", "zero"], extrapolate=False)
    window = [3, 1, 5, 3]
    loss, g, h = interpol.lcc_gauss_newton(moving, fixed, disp, weight, window=window, eps=1e-3, **kw)
    assert loss.shape == (2,) and g.shape == (2, *shape, 4) and h.shape == (2, *shape, 10)
    want = truth(moving, fixed, disp, weight, window=window, eps=1e-3, **kw)
    for a, b in zip((loss, g, h), want[:3]):
        torch.testing.assert_close(a, b, rtol=1e-11, atol=1e-13 * float(b.abs().max()))


def test_argument_errors():
    moving, fixed, disp, weight = problem((5, 6, 7), (4, 6, 5), 950, C=3)
    ok = dict(interpolation=1, bound="dct2")
    for bad in (4, 0, -3, [3, 2, 5], 3.0, True):
        with pytest.raises(ValueError, match="window"):
            interpol.lcc_gauss_newton(moving, fixed, disp, weight, window=bad, **ok)
    for bad in ([3, 5], [3, 5, 7, 9], []):
        with pytest.raises(ValueError, match="window"):
            interpol.lcc_gauss_newton(moving, fixed, disp, weight, window=bad, **ok)
    for bad in (0, 0.0, -1e-5, float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="eps"):
            interpol.lcc_gauss_newton(moving, fixed, disp, weight, eps=bad, **ok)
    with pytest.raises(ValueError, match="dtype and device"):
        interpol.lcc_gauss_newton(moving.float(), fixed, disp, weight, **ok)
    with pytest.raises(ValueError, match="dtype and device"):
        interpol.lcc_gauss_newton(moving, fixed, disp, weight.float(), **ok)
    with pytest.raises(ValueError, match="dtype and device"):
        interpol.lcc_gauss_newton(moving, fixed.to("meta"), disp, weight, **ok)
    with pytest.raises(ValueError, match="floating point"):
        interpol.lcc_gauss_newton(moving, fixed.long(), disp, weight, **ok)
    with pytest.raises(ValueError, match="channels"):
        interpol.lcc_gauss_newton(moving[:, :2], fixed, disp, weight, **ok)
    with pytest.raises(ValueError, match="spatial shape"):
        interpol.lcc_gauss_newton(moving, fixed[..., :3], disp, weight, **ok)
    with pytest.raises(ValueError, match="spatial shape"):
        interpol.lcc_gauss_newton(moving, fixed, disp[:, :2], weight, **ok)
    with pytest.raises(ValueError, match="spatial shape"):
        interpol.lcc_gauss_newton(moving, fixed, disp, weight[..., :3], **ok)
    with pytest.raises(ValueError, match="number of spatial dimensions"):
        interpol.lcc_gauss_newton(moving[0, 0], fixed[0], disp[0], None, **ok)
    with pytest.raises(ValueError, match="number of spatial dimensions"):
        interpol.lcc_gauss_newton(moving, fixed, torch.zeros(4, 6, 7, dtype=torch.float64), None, **ok)
    for bad in ("upper", "diag", 6, True):
        with pytest.raises(ValueError, match="hessian"):
            interpol.lcc_gauss_newton(moving, fixed, disp, weight, hessian=bad, **ok)
    for name in ("moving", "fixed", "disp", "weight"):
        args = dict(moving=moving, fixed=fixed, disp=disp, weight=weight)
        args[name] = args[name].clone().requires_grad_()
        with pytest.raises(RuntimeError, match="not differentiable"):
            interpol.lcc_gauss_newton(**args, **ok)
        with torch.no_grad():
            out = interpol.lcc_gauss_newton(**args, **ok)
        assert not any(t.requires_grad for t in out)
    from interpol import backend
    backend.jitfields = True
    try:
        with pytest.raises(RuntimeError, match="jitfields"):
            interpol.lcc_gauss_newton(moving, fixed, disp, weight, **ok)
    finally:
        backend.jitfields = False
