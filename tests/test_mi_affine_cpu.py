"""`interpol.mi_gauss_newton_affine`: the composed form (`torch_kernels.mi_gauss_newton_affine_composed`) in float64 on tiny lattices,
against autograd through `affine_grid` + `grid_pull` of a differentiable restatement of the loss; the properties of the joint
histogram; the helpers that tests/test_mi_affine_gpu.py shares.

gradient = d loss / d mat[:D] with the mask, the ranges and the fixed bins held constant: to 1e-10 relative to the largest entry.
The Hessian is a majoriser: exactly symmetric, smallest eigenvalue >= -1e-12 largest.

The recovery problem: a smooth moving image on 24^3 (sixteen random low-frequency cosines), the fixed image a NON-MONOTONE
function of its cubic pull through a known dyadic matrix, v -> 4 v (1 - v) of the normalised intensity: no sum of squares aligns
the two.  RECOVERY_ITERATIONS plain iterations mat -= solve(H, g) from the identity, order 1, 16 bins, the solve in float64; the
majoriser makes them short, safe steps (the loss falls at every one).  Measured with the composed form in float64: max |mat - true|
falls from 1.5 to RECOVERY_MEASURED times that; the test asserts half that reduction.
"""
import math

import pytest
import torch

import interpol
from interpol import ops, torch_kernels

CASES = [((5, 4, 6), (4, 5, 3)), ((7, 4), (6, 5)), ((7,), (9,))]          # moving -> fixed
IDS = ["x".join(map(str, s)) for _, s in CASES]
# dyadic entries, multiples of 1/32: every coordinate is exact in float32 (the matrices of tests/test_ssd_affine_cpu.py)
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


def binned(shape, bins, gen, lead=()):
    """values k + delta with integer k in 0 .. bins-1 and dyadic |delta| <= 1/4: under fixed_range = (0, bins - 1) no sample sits
    near a bin edge, so float32 and float64 pick the same bin"""
    k = torch.randint(0, bins, [*lead, *shape], generator=gen).double()
    delta = torch.randint(-8, 9, [*lead, *shape], generator=gen).double() / 32
    v = k + delta
    return v.clamp(0, bins - 1)                                             # (the ends of the range stay inside it: k + |delta|)


def problem(inshape, shape, seed, dtype=torch.float64, bins=8, B=None, weighted=True):
    """moving (B?, 1, *inshape) i.i.d. normal, fixed (B?, 1, *shape) = `binned`, weight (B?, *shape) uniform | None"""
    gen = torch.Generator().manual_seed(seed)
    lead = [] if B is None else [B]
    moving = torch.randn(*lead, 1, *inshape, generator=gen, dtype=torch.float64).to(dtype)
    fixed = binned(shape, bins, gen, [*lead, 1]).to(dtype)
    weight = torch.rand(*lead, *shape, generator=gen, dtype=torch.float64).to(dtype) if weighted else None
    return moving, fixed, weight


def restated_loss(moving, fixed, mat, weight, bins, moving_range, fixed_range, **kw):
    """minus the mutual information as a differentiable function of `mat`: unbatched float64 operands (moving (1,*in), fixed
    (1,*shape)); the mask, the ranges, the fixed bins and floor(u) are constants"""
    shape, dim = list(fixed.shape[1:]), mat.shape[-1] - 1
    I = interpol.grid_pull(moving, interpol.affine_grid(mat, shape), **kw)[0]
    with torch.no_grad():
        o = torch.stack(torch.meshgrid(*[torch.arange(n, dtype=torch.float64) for n in shape], indexing="ij"), -1)
        x = o @ mat[:, :dim].T + mat[:, dim]
        extrapolate = kw.get("extrapolate", True)
        mask = torch_kernels._mask(x, moving.shape[1:], int(extrapolate))
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


def close(got, want, rel=1e-10):
    return float((got - want).abs().max()) <= rel * max(float(want.abs().max()), 1e-300)


@pytest.mark.parametrize("extrapolate", [True, False], ids=["extrapolate", "in_view"])
@pytest.mark.parametrize("bound", ["dct2", "zero"])
@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_the_gradient_is_that_of_autograd_and_the_hessian_is_a_majoriser(case, order, bound, extrapolate):
    inshape, shape = CASES[case]
    dim = len(shape)
    for weighted, ranges in ((False, (None, None)), (True, ((-1.0, 1.5), (0.0, 7.0)))):
        moving, fixed, weight = problem(inshape, shape, 10 * case + weighted, bins=8, weighted=weighted)
        mat = matrix(dim, scale=0.25)
        kw = dict(interpolation=order, bound=bound, extrapolate=extrapolate)
        mi = dict(bins=8, moving_range=ranges[0], fixed_range=ranges[1])
        loss, grad, hess = interpol.mi_gauss_newton_affine(moving, fixed, mat, weight, **mi, **kw)
        m = mat.clone().requires_grad_(True)
        tl = restated_loss(moving, fixed, m, weight, 8, *ranges, **kw)
        tg, = torch.autograd.grad(tl, m)
        P = dim * (dim + 1)
        assert loss.shape == () and grad.shape == (dim, dim + 1) and hess.shape == (P, P)
        assert float(tg.abs().max()) > 0
        assert abs(float(loss - tl.detach())) <= 1e-12 and close(grad, tg), (float(loss - tl.detach()), float((grad - tg).abs().max()))
        assert torch.equal(hess, hess.mT)
        ev = torch.linalg.eigvalsh(hess)
        assert float(ev[0]) >= -1e-12 * float(ev[-1])
        l2, g2, h2 = interpol.mi_gauss_newton_affine(moving, fixed, mat, weight, hessian=False, **mi, **kw)
        assert h2 is None and torch.equal(l2, loss) and torch.equal(g2, grad)


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_the_histogram_sums_to_one_and_its_marginals_are_the_direct_sums(case):
    inshape, shape = CASES[case]
    dim, bins = len(shape), 9
    moving, fixed, weight = problem(inshape, shape, 30 + case, bins=bins)
    mat = matrix(dim, scale=0.25)
    kw = dict(interpolation=2, bound="dct2", extrapolate=False)
    loss, _, _, P = interpol.mi_gauss_newton_affine(moving, fixed, mat, weight, bins=bins, fixed_range=(0, bins - 1),
                                                    return_histogram=True, **kw)
    assert P.shape == (bins, bins) and bool((P >= 0).all()) and abs(float(P.sum()) - 1) <= 1e-14
    # the marginals from the samples, without the joint histogram
    o = torch.stack(torch.meshgrid(*[torch.arange(n, dtype=torch.float64) for n in shape], indexing="ij"), -1)
    x = o @ mat[:, :dim].T + mat[:, dim]
    omega = weight * torch_kernels._mask(x, inshape, 0).double()
    assert 0 < float((omega > 0).double().mean()) < 1                       # part of the lattice is out of view
    I = interpol.grid_pull(moving, x, **kw)[0]
    lo, hi = float(moving.min()), float(moving.max())
    u = 1.5 + ((I - lo) / (hi - lo)).clamp(0, 1) * (bins - 4)
    beta = torch_kernels.bspline3_taps(u - u.floor().clamp(1, bins - 3), 0)
    assert close(beta.sum(-1), torch.ones_like(u), 1e-14)
    j = (u.floor().clamp(1, bins - 3).long() - 1).unsqueeze(-1) + torch.arange(4)
    pm = torch.zeros(bins, dtype=torch.float64).index_add(0, j.reshape(-1), (omega.unsqueeze(-1) * beta).reshape(-1)) / omega.sum()
    k = (fixed[0] + 0.5).floor().long()
    pf = torch.zeros(bins, dtype=torch.float64).index_add(0, k.reshape(-1), omega.reshape(-1)) / omega.sum()
    assert close(P.sum(1), pm, 1e-13) and close(P.sum(0), pf, 1e-13)
    T = torch.where(P > 0, torch.log(P / (P.sum(1, keepdim=True) * P.sum(0, keepdim=True)).clamp_min(1e-300)), torch.zeros_like(P))
    assert abs(float(loss + (P * T).sum())) <= 1e-14 and float(loss) < 0


def test_a_constant_fixed_image_carries_no_information_and_no_weight_gives_zeros():
    moving, fixed, weight = problem((5, 4, 6), (4, 5, 3), 40)
    mat = matrix(3, scale=0.25)
    loss, grad, hess, P = interpol.mi_gauss_newton_affine(moving, torch.full_like(fixed, 3.0), mat, weight, bins=8, return_histogram=True)
    assert abs(float(loss)) <= 1e-14 and float(grad.abs().max()) <= 1e-14 and abs(float(P.sum()) - 1) <= 1e-14
    assert bool((P[:, 1:] == 0).all())                                      # a degenerate range: t_f = 0, every sample in bin 0
    out = interpol.mi_gauss_newton_affine(moving, fixed, mat, torch.zeros_like(weight), bins=8, return_histogram=True)
    assert all(bool((t == 0).all()) for t in out)
    # ... and so does a lattice that is out of view altogether
    far = mat.clone()
    far[:, -1] += 100.0
    out = interpol.mi_gauss_newton_affine(moving, fixed, far, weight, bins=8, extrapolate=False, return_histogram=True)
    assert all(bool((t == 0).all()) for t in out)


def test_invariance_to_a_flip_and_to_an_increasing_remap_of_the_fixed_intensities():
    """1 - fixed reverses the bins of the fixed side; an increasing AFFINE remap (the strictly monotone maps that send bins onto
    bins) leaves them where they are.  The fixed values sit at (k + delta) / (B - 1) with both ends present, so the ranges found by
    aminmax are [0, 1] and no sample sits near a bin edge."""
    bins = 8
    gen = torch.Generator().manual_seed(50)
    moving = torch.randn(1, 5, 4, 6, generator=gen, dtype=torch.float64)
    v = binned((4, 5, 3), bins, gen, [1])
    v.view(-1)[0], v.view(-1)[1] = 0.0, bins - 1.0
    fixed = v / (bins - 1)
    mat = matrix(3, scale=0.25)
    f = lambda fx: interpol.mi_gauss_newton_affine(moving, fx, mat, bins=bins, interpolation=3, return_histogram=True)
    ref = f(fixed)
    flip = f(1 - fixed)
    assert close(flip[3], ref[3].flip(-1), 1e-12) and abs(float(flip[0] - ref[0])) <= 1e-12 and close(flip[1], ref[1], 1e-12)
    remap = f(0.5 * fixed + 0.25)
    assert close(remap[3], ref[3], 1e-12) and abs(float(remap[0] - ref[0])) <= 1e-12 and close(remap[2], ref[2], 1e-12)


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_a_batch_of_matrices_is_one_call_per_matrix(case):
    inshape, shape = CASES[case]
    dim = len(shape)
    moving, fixed, weight = problem(inshape, shape, 70 + case, B=3)
    mats = torch.stack([matrix(dim, scale=s) for s in (0.25, 0.5, -0.125)])
    kw = dict(interpolation=3, bound="dct2", extrapolate=False, bins=8, return_histogram=True)
    got = interpol.mi_gauss_newton_affine(moving, fixed, mats, weight, **kw)
    P = dim * (dim + 1)
    assert got[0].shape == (3,) and got[1].shape == (3, dim, dim + 1) and got[2].shape == (3, P, P) and got[3].shape == (3, 8, 8)
    for b in range(3):
        one = interpol.mi_gauss_newton_affine(moving[b], fixed[b], mats[b], weight[b], **kw)
        assert all(close(g[b], o, 1e-13) for g, o in zip(got, one)), b
    # a shared moving image (batch 1) and a square matrix whose last row is ignored
    full = torch.cat([mats[0], torch.full((1, dim + 1), 7.0, dtype=torch.float64)])
    got = interpol.mi_gauss_newton_affine(moving[:1], fixed, full, weight, **kw)
    assert got[0].shape == (3,) and got[1].shape == (3, dim, dim + 1)
    for b in range(3):
        one = interpol.mi_gauss_newton_affine(moving[0], fixed[b], mats[0], weight[b], **kw)
        assert all(close(g[b], o, 1e-13) for g, o in zip(got, one)), b


def test_validation():
    moving, fixed, weight = problem((5, 4, 6), (4, 5, 3), 90)
    mat = matrix(3)
    f = interpol.mi_gauss_newton_affine
    with pytest.raises(ValueError, match="ONE channel"):
        f(moving.expand(2, 5, 4, 6), fixed.expand(2, 4, 5, 3), mat)
    with pytest.raises(ValueError, match="ONE channel"):
        f(moving, fixed.expand(3, 4, 5, 3), mat)
    for bins in (7, 0, -1, 8.0, True, None):
        with pytest.raises(ValueError, match="`bins` is an integer >= 8"):
            f(moving, fixed, mat, bins=bins)
    with pytest.raises(ValueError, match="pair of floats"):
        f(moving, fixed, mat, moving_range=1.0)
    with pytest.raises(ValueError, match="pair of floats"):
        f(moving, fixed, mat, fixed_range=(0.0, 1.0, 2.0))
    with pytest.raises(ValueError, match="floating point"):
        f(moving, fixed.long(), mat)
    with pytest.raises(ValueError, match="`fixed` must have the dtype and device of `mat`"):
        f(moving, fixed.float(), mat)
    with pytest.raises(ValueError, match="`weight` must have the dtype and device of `mat`"):
        f(moving, fixed, mat, weight.float())
    with pytest.raises(ValueError, match="sets the number of spatial dimensions"):
        f(moving, fixed, mat[:2])
    with pytest.raises(ValueError, match="`weight` must have the spatial shape of `fixed`"):
        f(moving, fixed, mat, weight[:3])
    with torch.enable_grad():
        with pytest.raises(RuntimeError, match="not differentiable"):
            f(moving, fixed, mat.clone().requires_grad_(True))
        with pytest.raises(RuntimeError, match="not differentiable"):
            f(moving.clone().requires_grad_(True), fixed, mat)
    with torch.no_grad():
        assert f(moving, fixed, mat.clone().requires_grad_(True))[2].shape == (12, 12)
    assert len(f(moving, fixed, mat)) == 3 and len(f(moving, fixed, mat, return_histogram=True)) == 4
    assert "mi_gauss_newton_affine" in interpol.api.__all__ and interpol.mi_gauss_newton_affine is f


def test_the_composed_form_serves_four_dimensions_mixed_orders_many_bins_and_16_bit():
    gen = torch.Generator().manual_seed(5)
    moving, fixed = torch.randn(1, 4, 3, 4, 3, generator=gen, dtype=torch.float64), binned((3, 4, 3, 2), 8, gen, [1])
    mat = torch.eye(5, dtype=torch.float64)[:4] + 0.0625 * torch.randn(4, 5, generator=gen, dtype=torch.float64)
    kw = dict(interpolation=[1, 2, 3, 1], bound="dct2", extrapolate=True)
    loss, grad, hess = interpol.mi_gauss_newton_affine(moving, fixed, mat, bins=100, **kw)
    m = mat.clone().requires_grad_(True)
    tl = restated_loss(moving, fixed, m, None, 100, None, None, **kw)
    tg, = torch.autograd.grad(tl, m)
    assert grad.shape == (4, 5) and hess.shape == (20, 20) and abs(float(loss - tl.detach())) <= 1e-12 and close(grad, tg)
    m3, f3, w3 = problem((5, 4, 6), (4, 5, 3), 91, dtype=torch.bfloat16)
    got = interpol.mi_gauss_newton_affine(m3, f3, matrix(3, torch.bfloat16, 0.25), w3, bins=8)
    want = interpol.mi_gauss_newton_affine(m3.double(), f3.double(), matrix(3, torch.float64, 0.25), w3.double(), bins=8)
    assert all(g.dtype == torch.bfloat16 for g in got)
    assert all(float((g.double() - w).abs().max()) <= 2e-2 * float(w.abs().max()) for g, w in zip(got, want))


# ---------------------------------------------------------------------------------------------------------------------
# recovery of a known matrix across a non-monotone change of intensity
# ---------------------------------------------------------------------------------------------------------------------
TRUE_MAT = [[1.0, 0.0625, -0.03125, 1.5], [-0.0625, 0.96875, 0.03125, -0.75], [0.03125, -0.0625, 1.03125, 1.25]]
RECOVERY_ITERATIONS = 30
RECOVERY_MEASURED = 0.0050                                                  # max |mat - true| after / before: 0.00747 / 1.5, composed form, float64


def field(dtype, device="cpu", seed=7, n=24, terms=16):
    """moving: sixteen random cosines of at most 2.5 periods across 24^3; fixed: 4 v (1 - v) of its cubic pull v (normalised to [0, 1])
    through TRUE_MAT on 24^3"""
    gen = torch.Generator().manual_seed(seed)
    inshape = (n, n, n)
    grid = interpol.identity_grid(inshape, dtype=torch.float64)
    moving = torch.zeros(inshape, dtype=torch.float64)
    for _ in range(terms):
        k = (torch.rand(3, generator=gen, dtype=torch.float64) * 2 - 1) * 2 * math.pi * 2.5 / n
        phase = float(torch.rand(1, generator=gen, dtype=torch.float64)) * 2 * math.pi
        moving += torch.cos((grid * k).sum(-1) + phase) * (0.5 + float(torch.rand(1, generator=gen, dtype=torch.float64)))
    moving = moving[None]
    true = torch.tensor(TRUE_MAT, dtype=torch.float64)
    coeff = interpol.spline_coeff_nd(moving, interpolation=3, bound="dct2", dim=3)
    v = interpol.grid_pull(coeff, interpol.affine_grid(true, inshape), interpolation=3, bound="dct2", extrapolate=True)
    v = (v - moving.min()) / (moving.max() - moving.min())
    fixed = 4 * v * (1 - v)
    return moving.to(dtype).to(device), fixed.to(dtype).to(device), true


def recover(moving, fixed, true, order=1, iterations=RECOVERY_ITERATIONS, bins=16):
    """max |mat - true| at the start and after each iteration mat -= solve(H, g) from the identity; the P x P solve in float64 on the host"""
    dtype, device = moving.dtype, moving.device
    mat = torch.eye(4, dtype=dtype, device=device)[:3]
    errors = [float((mat.double().cpu() - true).abs().max())]
    for _ in range(iterations):
        loss, g, H = interpol.mi_gauss_newton_affine(moving, fixed, mat, bins=bins, interpolation=order, bound="dct2", extrapolate=True)
        step = torch.linalg.solve(H.double().cpu(), g.reshape(-1).double().cpu())
        mat = mat - step.reshape(3, 4).to(dtype).to(device)
        errors.append(float((mat.double().cpu() - true).abs().max()))
    return errors


def test_recovery_of_a_known_matrix_float64():
    errors = recover(*field(torch.float64))
    print("recovery float64: max matrix error at the start %.3g, after %d iterations %.3g (ratio %.3g)"
          % (errors[0], RECOVERY_ITERATIONS, errors[-1], errors[-1] / errors[0]))
    assert errors[-1] / errors[0] <= recovery_bar()


def recovery_bar():
    """half the measured reduction: 1 - (1 - RECOVERY_MEASURED) / 2"""
    return 1 - (1 - RECOVERY_MEASURED) / 2


# ---------------------------------------------------------------------------------------------------------------------
# the truth and the allowance of the device tests (tests/test_mi_affine_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------
def quantum(N, wmax):
    """q = wmax 2^-min(52, 62 - ceil(log2 N)) of the fused histogram"""
    lg = 0
    while (1 << lg) < N:
        lg += 1
    return wmax * 2.0 ** -min(52, 62 - lg)


def truth_and_allowance(moving, fixed, mat, weight, tol, bins, moving_range, fixed_range, **kw):
    """The composed form in float64 on the CPU, fed the upcast operands as `ops` takes them (moving (B|1,1,*in), fixed (B|1,1,*shape),
    mat (B|1,D,D+1), weight None | (B|1,*shape)) -> (loss, gradient, hessian, P), and the allowance per entry.  An error e in I is
    an error (B - 4) e / (m_hi - m_lo) in u: with A = 1 + (B - 4) max|moving| / (m_hi - m_lo) per item, tol A takes the place of
    tol in the project's per-sample bar (tests/test_ssd_affine_cpu.py: `truth_and_allowance`), summed over the samples from the
    reference's own per-sample fields q_d = dI G_d and h_dd' = c G_d G_d':
        P[j, k]:        tol A P + N q / (2 W)                         (q: the quantum of the fixed-point histogram, half of it per update)
        gradient[d, e]: tol A sum_o (|q_d| + max|q_d|) |o~_e|;   hessian: tol A sum_o (|h_dd'| + max|h_dd'|) |o~_e o~_e'|
        loss:           tol A (|ref| + sum P |T|) + (N q / (2 W)) sum_{P > 0} |T|   (d loss / d P = -T up to terms that cancel)
    and the reference's own rounding: its T = log(P / (p_m p_f)) carries the relative roundings of P, p_m, p_f and of the log, an
    absolute dT = 4 * 2^-52, which is all there is where T vanishes (a lattice of one sample: P = p_m, p_f = 1); it enters the loss
    as dT (sum P = 1) and the gradient and the Hessian through |beta3'| and |beta3''| in the place of their products with T."""
    from interpol.codes import pad_codes
    from interpol.autograd import _options
    m, f, a = moving.double().cpu(), fixed.double().cpu(), mat.double().cpu()
    w = None if weight is None else weight.double().cpu()
    dim = a.shape[-1] - 1
    opt = _options(kw.get("bound", "dct2"), kw.get("interpolation", 1), kw.get("extrapolate", True))
    bound, order = pad_codes(opt[0], dim), pad_codes(opt[1], dim)
    shape = list(f.shape[2:])
    B = max(m.shape[0], f.shape[0], a.shape[0], 1 if w is None else w.shape[0])
    ranges = torch_kernels.mi_ranges(m, f, w, moving_range, fixed_range, B)
    want = torch_kernels.mi_gauss_newton_affine_composed(m, f, a, w, ranges, bound, order, int(opt[2]), True, bins, True)
    loss, _, _, P = want
    N = 1
    for n in shape:
        N *= n
    # the per-sample fields of the reference
    o = torch.stack(torch.meshgrid(*[torch.arange(n, dtype=torch.float64) for n in shape], indexing="ij"), -1)
    x = torch.stack([o @ ab[:, :dim].T + ab[:, dim] for ab in a])
    I = ops.grid_pull(m, x, bound, order, int(opt[2]))[:, 0].expand([B] + shape)
    G = ops.grid_grad(m, x, bound, order, int(opt[2]))[:, 0].expand([B] + shape + [dim])
    mask = torch_kernels._mask(x, m.shape[2:], int(opt[2]))
    omega = torch.ones([1] + shape, dtype=torch.float64) if w is None else w
    if mask is not None:
        omega = omega * mask.double()
    omega = omega.expand([B] + shape)
    W = omega.reshape(B, -1).sum(1)
    j0, fr, clamped, k = torch_kernels.mi_bins(I, f[:, 0], ranges, bins)
    pm, pf = P.sum(2, keepdim=True), P.sum(1, keepdim=True)
    T = torch.where(P > 0, torch.log(torch.where(P > 0, P / (pm * pf).clamp_min(1e-300), torch.ones_like(P))), torch.zeros_like(P))
    idx = ((j0.unsqueeze(-1) + torch.arange(4)) * bins + k.unsqueeze(-1)) + (torch.arange(B) * bins * bins).reshape([B] + [1] * (dim + 1))
    Tt = T.reshape(-1)[idx]
    sc = torch.where(clamped, torch.zeros_like(I), (bins - 4) * ranges[:, 1].reshape([B] + [1] * dim).expand_as(I))
    wn = omega / W.clamp_min(1e-300).reshape([B] + [1] * dim)
    dI = (wn * sc) * (torch_kernels.bspline3_taps(fr, 1) * Tt).sum(-1)
    c = (wn * sc) * sc * (torch_kernels.bspline3_taps(fr, 2) * Tt.abs()).sum(-1)
    q = (dI.unsqueeze(-1) * G).reshape(B, N, dim).abs()
    dT = 4 * 2.0 ** -52
    q0 = ((wn * sc) * torch_kernels.bspline3_taps(fr, 1).abs().sum(-1)).unsqueeze(-1) * G.abs()
    c0 = (wn * sc) * sc * torch_kernels.bspline3_taps(fr, 2).sum(-1)
    A = 1 + (bins - 4) * m.reshape(m.shape[0], -1).abs().amax(1).expand(B) * ranges[:, 1]
    tA = tol * A
    ot = torch.cat([o, torch.ones_like(o[..., :1])], -1).reshape(-1, dim + 1)
    q = q + q.amax(1, keepdim=True)
    ag = tA.reshape(B, 1, 1) * torch.einsum("bnd,ne->bde", q, ot) + dT * torch.einsum("bnd,ne->bde", q0.reshape(B, N, dim), ot)
    h = (c.reshape(B, N, 1, 1) * G.reshape(B, N, dim, 1) * G.reshape(B, N, 1, dim)).abs()
    h = h + h.amax(1, keepdim=True)
    mo = ot[:, :, None] * ot[:, None, :]
    Pn = dim * (dim + 1)
    h0 = (c0.reshape(B, N, 1, 1) * G.reshape(B, N, dim, 1) * G.reshape(B, N, 1, dim)).abs()
    ah = (tA.reshape(B, 1, 1) * torch.einsum("bnij,nef->biejf", h, mo).reshape(B, Pn, Pn)
          + dT * torch.einsum("bnij,nef->biejf", h0, mo).reshape(B, Pn, Pn))
    wmax = ranges[:, 4]
    quant = torch.tensor([N * quantum(N, float(wm)) for wm in wmax]) / (2 * W.clamp_min(1e-300))
    aP = tA.reshape(B, 1, 1) * P + quant.reshape(B, 1, 1)
    al = tA * (loss.abs() + (P * T.abs()).reshape(B, -1).sum(1)) + quant * T.abs().reshape(B, -1).sum(1) + dT
    return want, (al, ag, ah, aP)


def worst_ratio(got, want, allow):
    """max over the entries of |got - want| / allowance (0 / 0 counts as 0)"""
    err = (got.double().cpu() - want).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / allow).max())
