"""`interpol.mi_gauss_newton`: the composed form (`torch_kernels.mi_gauss_newton_composed`) in float64 on tiny lattices, against
autograd through `grid_pull(..., displacement=True)` of a differentiable restatement of the loss; the per-voxel majoriser; the
agreement with `mi_gauss_newton_affine` on the dense field of an affine matrix; the helpers that tests/test_mi_gpu.py shares.

gradient = d loss / d disp with the mask, the ranges, the fixed bins and floor(u) held constant: to 1e-10 relative to the largest
entry (`close` of tests/test_mi_affine_cpu.py).  Each D x D block of the Hessian is positive semi-definite: smallest eigenvalue
>= -1e-14 largest.

The descent problem: the 24^3 images of tests/test_mi_affine_cpu.py (`field`: the fixed image is 4 v (1 - v) of the pulled moving
image, a NON-MONOTONE change of intensity).  DESCENT_ITERATIONS Gauss-Newton steps from disp = 0, 16 bins, order 1:

    loss, g, H = mi_gauss_newton(moving, fixed, disp, bins=16);  g += regulariser(disp, membrane=lam, bound='dct2')
    disp -= regulariser_solve(g, H, membrane=lam, bound='dct2', max_iter=32)

with lam = the mean of the diagonal Hessian entries at disp = 0.  loss + regulariser_energy falls at every step; measured with the
composed form in float64 it goes from DESCENT_MEASURED[0] to DESCENT_MEASURED[1]; the device test asserts half that fall.
"""
import pytest
import torch

import interpol
from interpol import ops, torch_kernels
from interpol.sepgrid import AffineGrid
import test_mi_affine_cpu as aff

CASES, IDS, close = aff.CASES, aff.IDS, aff.close


def dyadic_noise(shape, dim, gen, sigma=2.0, lead=()):
    """i.i.d. normal displacements of standard deviation `sigma`, rounded to multiples of 1/32: o + disp is exact in float32"""
    return (torch.randn(*lead, *shape, dim, generator=gen, dtype=torch.float64) * sigma * 32).round() / 32


def dyadic_smooth(shape, dim, amplitude=1.5, shift=0.0):
    """a smooth displacement (one cosine per component across the lattice) plus `shift`, rounded to multiples of 1/32"""
    o = interpol.identity_grid(shape, dtype=torch.float64)
    cols = []
    for d in range(dim):
        phase = sum(o[..., e] * (0.9 + 0.4 * ((d + e) % 3)) / max(shape[e], 2) for e in range(dim))
        cols.append(amplitude * torch.cos(2.0 * phase + d) + shift)
    return (torch.stack(cols, -1) * 32).round() / 32


def restated_loss(moving, fixed, disp, weight, bins, moving_range, fixed_range, **kw):
    """minus the mutual information as a differentiable function of `disp`: unbatched float64 operands (moving (1,*in), fixed
    (1,*shape), disp (*shape,D)); the mask, the ranges, the fixed bins and floor(u) are constants"""
    shape = list(fixed.shape[1:])
    I = interpol.grid_pull(moving, disp, displacement=True, **kw)[0]
    with torch.no_grad():
        x = disp + interpol.identity_grid(shape, dtype=torch.float64)
        mask = torch_kernels._mask(x, moving.shape[1:], int(kw.get("extrapolate", True)))
        omega = torch.ones(shape, dtype=torch.float64) if weight is None else weight.clone()
        if mask is not None:
            omega = omega * mask.double()
        ranges = torch_kernels.mi_ranges(moving[None], fixed[None], None, moving_range, fixed_range, 1)[0]
        k = ((((fixed[0] - ranges[2]) * ranges[3]).clamp(0, 1)) * (bins - 1) + 0.5).floor().long().clamp(0, bins - 1)
    u = 1.5 + ((I - ranges[0]) * ranges[1]).clamp(0, 1) * (bins - 4)
    fl = u.detach().floor().clamp(1, bins - 3)
    beta = torch_kernels.bspline3_taps(u - fl, 0)
    idx = (fl.long() - 1).unsqueeze(-1) + torch.arange(4)
    H = torch.zeros(bins * bins, dtype=torch.float64).index_add(0, (idx * bins + k.unsqueeze(-1)).reshape(-1),
                                                               (omega.unsqueeze(-1) * beta).reshape(-1)).reshape(bins, bins)
    P = H / omega.sum()
    pm, pf = P.sum(1, keepdim=True), P.sum(0, keepdim=True)
    pos = P > 0
    return -(P[pos] * torch.log(P[pos] / (pm * pf)[pos])).sum()


@pytest.mark.parametrize("extrapolate", [True, False], ids=["extrapolate", "in_view"])
@pytest.mark.parametrize("bound", ["dct2", "zero", "dft"])
@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_the_gradient_is_that_of_autograd_and_every_block_of_the_hessian_is_a_majoriser(case, order, bound, extrapolate):
    inshape, shape = CASES[case]
    dim = len(shape)
    for weighted, ranges in ((False, (None, None)), (True, ((-1.0, 1.5), (0.0, 7.0)))):
        moving, fixed, weight = aff.problem(inshape, shape, 10 * case + weighted, bins=8, weighted=weighted)
        disp = dyadic_noise(shape, dim, torch.Generator().manual_seed(100 + case), sigma=0.75)
        kw = dict(interpolation=order, bound=bound, extrapolate=extrapolate)
        mi = dict(bins=8, moving_range=ranges[0], fixed_range=ranges[1])
        loss, grad, hess = interpol.mi_gauss_newton(moving, fixed, disp, weight, **mi, **kw)
        u = disp.clone().requires_grad_(True)
        tl = restated_loss(moving, fixed, u, weight, 8, *ranges, **kw)
        tg, = torch.autograd.grad(tl, u)
        K = dim * (dim + 1) // 2
        assert loss.shape == () and grad.shape == (*shape, dim) and hess.shape == (*shape, K)
        assert float(tg.abs().max()) > 0
        assert abs(float(loss - tl.detach())) <= 1e-12 and close(grad, tg), (float(loss - tl.detach()), float((grad - tg).abs().max()))
        ev = torch.linalg.eigvalsh(torch_kernels.symmetric_matrix(hess, dim))
        assert bool((ev[..., 0] >= -1e-14 * ev[..., -1]).all()) and float(ev.max()) > 0
        l1, g1, h1 = interpol.mi_gauss_newton(moving, fixed, disp, weight, hessian="diagonal", **mi, **kw)
        assert h1.shape == (*shape, dim) and torch.equal(h1, hess[..., :dim]) and torch.equal(l1, loss) and torch.equal(g1, grad)
        l2, g2, h2 = interpol.mi_gauss_newton(moving, fixed, disp, weight, hessian=None, **mi, **kw)
        assert h2 is None and torch.equal(l2, loss) and torch.equal(g2, grad)
        if not extrapolate:                                                 # out-of-view samples: zero gradient and Hessian
            x = disp + interpol.identity_grid(shape, dtype=torch.float64)
            out = ~torch_kernels._mask(x, inshape, 0)
            assert bool(out.any()) and bool((grad[out] == 0).all()) and bool((hess[out] == 0).all())


@pytest.mark.parametrize("order", [1, 3])
@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_on_the_field_of_an_affine_matrix_it_agrees_with_the_affine_term(case, order):
    inshape, shape = CASES[case]
    dim, bins = len(shape), 8
    moving, fixed, weight = aff.problem(inshape, shape, 200 + case, bins=bins)
    mat = aff.matrix(dim, scale=0.25)
    o = interpol.identity_grid(shape, dtype=torch.float64)
    disp = AffineGrid(mat, shape).dense().reshape(*shape, dim) - o
    kw = dict(interpolation=order, bound="dct2", extrapolate=False, bins=bins, fixed_range=(0, bins - 1), return_histogram=True)
    la, ga, ha, Pa = interpol.mi_gauss_newton_affine(moving, fixed, mat, weight, **kw)
    loss, grad, hess, P = interpol.mi_gauss_newton(moving, fixed, disp, weight, **kw)
    assert close(loss, la, 1e-12) and close(P, Pa, 1e-12)
    ot = torch.cat([o, torch.ones_like(o[..., :1])], -1).reshape(-1, dim + 1)
    assert close(torch.einsum("nd,ne->de", grad.reshape(-1, dim), ot), ga)
    S = torch_kernels.symmetric_matrix(hess, dim).reshape(-1, dim, dim)
    Pn = dim * (dim + 1)
    assert close(torch.einsum("ndk,ne,nf->dekf", S, ot, ot).reshape(Pn, Pn), ha)


def test_a_constant_fixed_image_carries_no_information_and_no_weight_gives_zeros():
    moving, fixed, weight = aff.problem((5, 4, 6), (4, 5, 3), 40)
    disp = dyadic_noise((4, 5, 3), 3, torch.Generator().manual_seed(41), sigma=0.5)
    loss, grad, hess, P = interpol.mi_gauss_newton(moving, torch.full_like(fixed, 3.0), disp, weight, bins=8, return_histogram=True)
    assert abs(float(loss)) <= 1e-14 and float(grad.abs().max()) <= 1e-14 and abs(float(P.sum()) - 1) <= 1e-14
    assert bool((P[:, 1:] == 0).all())                                      # a degenerate range: t_f = 0, every sample in bin 0
    out = interpol.mi_gauss_newton(moving, fixed, disp, torch.zeros_like(weight), bins=8, return_histogram=True)
    assert all(bool((t == 0).all()) for t in out)
    # ... and so does a lattice that is out of view altogether
    out = interpol.mi_gauss_newton(moving, fixed, disp + 100.0, weight, bins=8, extrapolate=False, return_histogram=True)
    assert all(bool((t == 0).all()) for t in out)


def test_the_loss_is_invariant_to_an_increasing_remap_of_the_fixed_intensities():
    """An increasing AFFINE remap (the strictly monotone maps that send bins onto bins) leaves every sample in its bin; the flip
    1 - fixed reverses the bins.  The fixed values are those of tests/test_mi_affine_cpu.py: the ranges found by aminmax are [0, 1]."""
    bins = 8
    gen = torch.Generator().manual_seed(50)
    moving = torch.randn(1, 5, 4, 6, generator=gen, dtype=torch.float64)
    v = aff.binned((4, 5, 3), bins, gen, [1])
    v.view(-1)[0], v.view(-1)[1] = 0.0, bins - 1.0
    fixed = v / (bins - 1)
    disp = dyadic_noise((4, 5, 3), 3, gen, sigma=0.5)
    f = lambda fx: interpol.mi_gauss_newton(moving, fx, disp, bins=bins, interpolation=3, return_histogram=True)
    ref = f(fixed)
    remap = f(0.5 * fixed + 0.25)
    assert close(remap[3], ref[3], 1e-12) and abs(float(remap[0] - ref[0])) <= 1e-12
    assert close(remap[1], ref[1], 1e-12) and close(remap[2], ref[2], 1e-12)
    flip = f(1 - fixed)
    assert close(flip[3], ref[3].flip(-1), 1e-12) and abs(float(flip[0] - ref[0])) <= 1e-12 and close(flip[1], ref[1], 1e-12)


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_a_batch_is_one_call_per_item(case):
    inshape, shape = CASES[case]
    dim = len(shape)
    moving, fixed, weight = aff.problem(inshape, shape, 70 + case, B=3)
    disp = dyadic_noise(shape, dim, torch.Generator().manual_seed(71), sigma=0.75, lead=(3,))
    kw = dict(interpolation=3, bound="dct2", extrapolate=False, bins=8, return_histogram=True)
    got = interpol.mi_gauss_newton(moving, fixed, disp, weight, **kw)
    K = dim * (dim + 1) // 2
    assert got[0].shape == (3,) and got[1].shape == (3, *shape, dim) and got[2].shape == (3, *shape, K) and got[3].shape == (3, 8, 8)
    for b in range(3):
        one = interpol.mi_gauss_newton(moving[b], fixed[b], disp[b], weight[b], **kw)
        assert all(close(g[b], o, 1e-13) for g, o in zip(got, one)), b
    # a shared moving image and a shared field (no batch): nothing is copied, the batch is that of `fixed`
    got = interpol.mi_gauss_newton(moving[0], fixed, disp[0], weight, **kw)
    assert got[0].shape == (3,) and got[1].shape == (3, *shape, dim)
    for b in range(3):
        one = interpol.mi_gauss_newton(moving[0], fixed[b], disp[0], weight[b], **kw)
        assert all(close(g[b], o, 1e-13) for g, o in zip(got, one)), b


def test_validation():
    moving, fixed, weight = aff.problem((5, 4, 6), (4, 5, 3), 90)
    disp = torch.zeros(4, 5, 3, 3, dtype=torch.float64)
    f = interpol.mi_gauss_newton
    with pytest.raises(ValueError, match="mi_gauss_newton: `moving` and `fixed` must have ONE channel"):
        f(moving.expand(2, 5, 4, 6), fixed.expand(2, 4, 5, 3), disp)
    with pytest.raises(ValueError, match="mi_gauss_newton: `moving` and `fixed` must have the same number of channels"):
        f(moving, fixed.expand(3, 4, 5, 3), disp)
    for bins in (7, 0, -1, 8.0, True, None):
        with pytest.raises(ValueError, match="mi_gauss_newton: `bins` is an integer >= 8"):
            f(moving, fixed, disp, bins=bins)
    with pytest.raises(ValueError, match="mi_gauss_newton: `moving_range` is None or a pair of floats"):
        f(moving, fixed, disp, moving_range=1.0)
    with pytest.raises(ValueError, match="mi_gauss_newton: `fixed_range` is None or a pair of floats"):
        f(moving, fixed, disp, fixed_range=(0.0, 1.0, 2.0))
    with pytest.raises(ValueError, match="mi_gauss_newton: .*floating point"):
        f(moving, fixed.long(), disp)
    with pytest.raises(ValueError, match="mi_gauss_newton: `fixed` must have the dtype and device of `disp`"):
        f(moving, fixed.float(), disp)
    with pytest.raises(ValueError, match="mi_gauss_newton: `weight` must have the dtype and device of `disp`"):
        f(moving, fixed, disp, weight.float())
    with pytest.raises(ValueError, match="mi_gauss_newton: the last dimension of `disp`"):
        f(moving, fixed, disp[..., :0])
    with pytest.raises(ValueError, match="mi_gauss_newton: `fixed` and `disp` must share the spatial shape"):
        f(moving, fixed, disp[:3])
    with pytest.raises(ValueError, match="mi_gauss_newton: `weight` must have the spatial shape of `fixed`"):
        f(moving, fixed, disp, weight[:3])
    with pytest.raises(ValueError, match="mi_gauss_newton: `hessian` is 'full', 'diagonal' or None"):
        f(moving, fixed, disp, hessian=True)
    with torch.enable_grad():
        with pytest.raises(RuntimeError, match="mi_gauss_newton is not differentiable"):
            f(moving, fixed, disp.clone().requires_grad_(True))
        with pytest.raises(RuntimeError, match="mi_gauss_newton is not differentiable"):
            f(moving.clone().requires_grad_(True), fixed, disp)
    with torch.no_grad():
        assert f(moving, fixed, disp.clone().requires_grad_(True))[2].shape == (4, 5, 3, 6)
    assert len(f(moving, fixed, disp)) == 3 and len(f(moving, fixed, disp, return_histogram=True)) == 4
    assert "mi_gauss_newton" in interpol.api.__all__ and interpol.mi_gauss_newton is f
    # the affine term keeps its own name in the messages of the shared checks
    with pytest.raises(ValueError, match="mi_gauss_newton_affine: `bins` is an integer >= 8"):
        interpol.mi_gauss_newton_affine(moving, fixed, aff.matrix(3), bins=7)
    with pytest.raises(ValueError, match="mi_gauss_newton_affine: `fixed_range` is None or a pair of floats"):
        interpol.mi_gauss_newton_affine(moving, fixed, aff.matrix(3), fixed_range=3)


def test_the_composed_form_serves_four_dimensions_mixed_orders_many_bins_and_16_bit():
    gen = torch.Generator().manual_seed(5)
    moving, fixed = torch.randn(1, 4, 3, 4, 3, generator=gen, dtype=torch.float64), aff.binned((3, 4, 3, 2), 8, gen, [1])
    disp = dyadic_noise((3, 4, 3, 2), 4, gen, sigma=0.5)
    kw = dict(interpolation=[1, 2, 3, 1], bound="dct2", extrapolate=True)
    loss, grad, hess = interpol.mi_gauss_newton(moving, fixed, disp, bins=100, **kw)
    u = disp.clone().requires_grad_(True)
    tl = restated_loss(moving, fixed, u, None, 100, None, None, **kw)
    tg, = torch.autograd.grad(tl, u)
    assert grad.shape == (3, 4, 3, 2, 4) and hess.shape == (3, 4, 3, 2, 10) and abs(float(loss - tl.detach())) <= 1e-12 and close(grad, tg)
    m3, f3, w3 = aff.problem((5, 4, 6), (4, 5, 3), 91, dtype=torch.bfloat16)
    d3 = dyadic_noise((4, 5, 3), 3, gen, sigma=0.5).to(torch.bfloat16)
    got = interpol.mi_gauss_newton(m3, f3, d3, w3, bins=8)
    want = interpol.mi_gauss_newton(m3.double(), f3.double(), d3.double(), w3.double(), bins=8)
    assert all(g.dtype == torch.bfloat16 for g in got)
    assert all(float((g.double() - w).abs().max()) <= 2e-2 * float(w.abs().max()) for g, w in zip(got, want))


# ---------------------------------------------------------------------------------------------------------------------
# descent across a non-monotone change of intensity
# ---------------------------------------------------------------------------------------------------------------------
DESCENT_ITERATIONS = 12
DESCENT_MEASURED = (-0.0364389, -0.434924)                                  # loss + energy at disp = 0 and after 12 steps: composed form, float64


def descend(moving, fixed, iterations=DESCENT_ITERATIONS, bins=16):
    """loss + regulariser_energy at disp = 0 and after each Gauss-Newton step (module docstring), as floats"""
    shape = list(fixed.shape[1:])
    disp = torch.zeros(*shape, 3, dtype=moving.dtype, device=moving.device)
    lam, totals = None, []
    for it in range(iterations + 1):
        loss, g, H = interpol.mi_gauss_newton(moving, fixed, disp, bins=bins)
        if lam is None:
            lam = float(H[..., :3].double().mean())
        totals.append(float(loss) + float(interpol.regulariser_energy(disp, membrane=lam, bound="dct2")))
        if it == iterations:
            break
        g = g + interpol.regulariser(disp, membrane=lam, bound="dct2")
        disp = disp - interpol.regulariser_solve(g, H, membrane=lam, bound="dct2", max_iter=32)
    return totals


def descent_bar():
    """half the measured fall"""
    return (DESCENT_MEASURED[1] - DESCENT_MEASURED[0]) / 2


def test_descent_float64():
    moving, fixed, _ = aff.field(torch.float64)
    totals = descend(moving, fixed)
    print("descent float64: loss + energy %s" % " ".join("%.6g" % t for t in totals))
    assert all(b < a for a, b in zip(totals, totals[1:])), totals
    assert abs(totals[0] - DESCENT_MEASURED[0]) <= 5e-4 * abs(DESCENT_MEASURED[0])
    assert abs(totals[-1] - DESCENT_MEASURED[1]) <= 5e-4 * abs(DESCENT_MEASURED[1])
    assert totals[-1] - totals[0] <= descent_bar() < 0


# ---------------------------------------------------------------------------------------------------------------------
# the truth and the allowance of the device tests (tests/test_mi_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------
def truth_and_allowance(moving, fixed, disp, weight, tol, bins, moving_range, fixed_range, hessian="full", **kw):
    """The composed form in float64 on the CPU, fed the upcast operands as `ops` takes them (moving (B|1,1,*in), fixed (B|1,1,*shape),
    disp (B|1,*shape,D), weight None | (B|1,*shape)) -> (loss, gradient, hessian, P), the allowance per entry and `keep` (B,*shape):
    the samples the fields are compared at.

    The loss and P: the per-entry terms of tests/test_mi_affine_cpu.py (`truth_and_allowance`) unchanged -- with A = 1 + (B - 4)
    max|moving| m_sc per item, P: tol A P + N q / (2 W); loss: tol A (|ref| + sum P |T|) + (N q / (2 W)) sum_{P > 0} |T| + dT.
    The fields: its per-sample summands before the contraction with the sample index,
        gradient[o, d]: tol A (|q_d(o)| + max_o |q_d|) + dT q0_d(o),   q_d = dI G_d,   q0_d = (omega / W) s sum_j |beta3'| |G_d|
        hessian[o, k]:  tol A (|h_k(o)| + max_o |h_k|) + dT h0_k(o),   h_k = c G_d G_e, h0_k = (omega / W) s^2 sum_j |beta3''| |G_d G_e|
    dT = 4 * 2^-52: the reference's own rounding of T.

    A correction to that derivation, from the number format of the histogram alone: the two fields read T = log(P) - log(p_m) -
    log(p_f), and each update of the fixed-point histogram is rounded to the quantum q: a bin that n[j, k] samples update carries
    e_q[j, k] = n[j, k] q / (2 W) (the bar of P grants N q / (2 W), its largest value), a row, a column and the total the sums of
    their bins'.  Through the logarithm that is
        dTq[j, k] = 2 e_q / P + sum_k e_q / p_m + sum_j e_q / p_f + sum_jk e_q     (2 x bounds -log(1 - x) for x = e_q / P < 1/2; |T| + 1
                                                                 beyond, where the bin may round to empty; 0 where P = 0)
    per bin -- not small where a bin is nearly empty: a bin of P = 2.3e-12 filled by taps at the end of the B-spline's support
    under weights of 1e-4.  It enters the sample as |beta3'| and |beta3''| enter through dT:
        gradient[o, d] += (omega / W) s sum_j |beta3'| dTq[j, k(o)] |G_d|,   hessian[o, k] += (omega / W) s^2 sum_j |beta3''| dTq |G_d G_e|.
    Without it the float64 case "B=3, shared moving image, batched weight" of tests/test_mi_gpu.py came to 2.25 of its bar in the
    Hessian (3.3e-13 against 1.6e-13 at one voxel); the composed form in float64 on the CPU with nothing changed but its updates
    rounded to the quantum comes to 2.13 at the same voxel, and the float32 composed form on the CPU misses a 1e-11 bar by
    construction: the miss is the format's, not the kernels'.  The affine term contracts these summands over the lattice, where
    N max|q| hides the term.
    The only discontinuity of a per-voxel term is the clamp of t_m (s jumps to 0): samples whose float64 raw = (I - m_lo) m_sc lies
    within 4 tol max|moving| m_sc of 0 or 1 are left out of `keep`; from the truth alone they number at most max(1, N / 1000) per
    item (asserted here)."""
    from interpol.codes import pad_codes
    from interpol.autograd import _options
    m, f, u = moving.double().cpu(), fixed.double().cpu(), disp.double().cpu()
    w = None if weight is None else weight.double().cpu()
    dim = u.shape[-1]
    opt = _options(kw.get("bound", "dct2"), kw.get("interpolation", 1), kw.get("extrapolate", True))
    bound, order = pad_codes(opt[0], dim), pad_codes(opt[1], dim)
    shape = list(f.shape[2:])
    B = max(m.shape[0], f.shape[0], u.shape[0], 1 if w is None else w.shape[0])
    ranges = torch_kernels.mi_ranges(m, f, w, moving_range, fixed_range, B)
    want = torch_kernels.mi_gauss_newton_composed(m, f, u, w, ranges, bound, order, int(opt[2]), hessian, bins, True)
    loss, _, _, P = want
    N = 1
    for n in shape:
        N *= n
    # the per-sample fields of the reference
    I = ops.grid_pull(m, u, bound, order, int(opt[2]), displacement=True)[:, 0].expand([B] + shape)
    G = ops.grid_grad(m, u, bound, order, int(opt[2]), displacement=True)[:, 0].expand([B] + shape + [dim])
    mask = torch_kernels._mask(u + interpol.identity_grid(shape, dtype=torch.float64), m.shape[2:], int(opt[2]))
    omega = torch.ones([1] + shape, dtype=torch.float64) if w is None else w
    if mask is not None:
        omega = omega * mask.double()
    omega = omega.expand([B] + shape)
    W = omega.reshape(B, -1).sum(1)
    j0, fr, clamped, k = torch_kernels.mi_bins(I, f[:, 0], ranges, bins)
    pm, pf = P.sum(2, keepdim=True), P.sum(1, keepdim=True)
    T = torch.where(P > 0, torch.log(torch.where(P > 0, P / (pm * pf).clamp_min(1e-300), torch.ones_like(P))), torch.zeros_like(P))
    col = lambda t: t.reshape([B] + [1] * dim)
    sc = torch.where(clamped, torch.zeros_like(I), (bins - 4) * col(ranges[:, 1]).expand_as(I))
    wn = omega / col(W.clamp_min(1e-300))
    dT = 4 * 2.0 ** -52
    mmax = m.reshape(m.shape[0], -1).abs().amax(1).expand(B)
    A = 1 + (bins - 4) * mmax * ranges[:, 1]
    tA = tol * A
    pairs = [(d, d) for d in range(dim)]
    if hessian == "full":
        pairs += [(d, e) for d in range(dim) for e in range(d + 1, dim)]
    wmax = ranges[:, 4]
    quant = torch.tensor([N * aff.quantum(N, float(wm)) for wm in wmax]) / (2 * W.clamp_min(1e-300))
    # the quantum in T, per bin: T = log(P) - log(p_m) - log(p_f) with P = H / W
    idx = ((j0.unsqueeze(-1) + torch.arange(4)) * bins + k.unsqueeze(-1)) + (torch.arange(B) * bins * bins).reshape([B] + [1] * (dim + 1))
    cnt = torch.zeros(B * bins * bins, dtype=torch.float64).index_add_(0, idx.reshape(-1), torch.ones(idx.numel(), dtype=torch.float64))
    eq = cnt.reshape(B, bins, bins) * (quant / N).reshape(B, 1, 1)          # n[j, k] q / (2 W): half a quantum per update of the bin
    xq = eq / P.clamp_min(1e-300)
    dTq = (torch.where(xq < 0.5, 2 * xq, T.abs() + 1) + eq.sum(2, keepdim=True) / pm.clamp_min(1e-300)
           + eq.sum(1, keepdim=True) / pf.clamp_min(1e-300) + eq.sum((1, 2), keepdim=True))
    dTq = torch.where(P > 0, dTq, torch.zeros_like(P))
    dTt = dTq.reshape(-1)[idx]                                              # (B,*shape,4)
    q = want[1].abs()
    q0 = ((wn * sc) * torch_kernels.bspline3_taps(fr, 1).abs().sum(-1)).unsqueeze(-1) * G.abs()
    qq = ((wn * sc) * (torch_kernels.bspline3_taps(fr, 1).abs() * dTt).sum(-1)).unsqueeze(-1) * G.abs()
    flat_max = lambda t: t.reshape(B, N, -1).amax(1).reshape([B] + [1] * dim + [t.shape[-1]])
    ag = col(tA).unsqueeze(-1) * (q + flat_max(q)) + dT * q0 + qq
    ah = None
    if hessian is not None:
        h = want[2].abs()
        c0 = (wn * sc) * sc * torch_kernels.bspline3_taps(fr, 2).sum(-1)
        cq = (wn * sc) * sc * (torch_kernels.bspline3_taps(fr, 2) * dTt).sum(-1)
        h0 = torch.stack([c0 * (G[..., d] * G[..., e]).abs() for d, e in pairs], -1)
        hq = torch.stack([cq * (G[..., d] * G[..., e]).abs() for d, e in pairs], -1)
        ah = col(tA).unsqueeze(-1) * (h + flat_max(h)) + dT * h0 + hq
    aP = tA.reshape(B, 1, 1) * P + quant.reshape(B, 1, 1)
    al = tA * (loss.abs() + (P * T.abs()).reshape(B, -1).sum(1)) + quant * T.abs().reshape(B, -1).sum(1) + dT
    # the clamp of t_m
    raw = (I - col(ranges[:, 0])) * col(ranges[:, 1])
    margin = col(4 * tol * mmax * ranges[:, 1])
    keep = ~(((raw - 0).abs() <= margin) | ((raw - 1).abs() <= margin))
    left_out = (~keep).reshape(B, -1).sum(1)
    assert int(left_out.max()) <= max(1, N // 1000), (left_out.tolist(), N)
    return want, (al, ag, ah, aP), keep


def worst_field_ratio(got, want, allow, keep):
    """max over the kept samples of |got - want| / allowance (0 / 0 counts as 0)"""
    err = (got.double().cpu() - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / allow)
    return float(ratio[keep].max()) if bool(keep.any()) else 0.0
