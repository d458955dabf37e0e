"""`interpol.ssd_gauss_newton` on the CPU: the composed form (interpol/torch_kernels.py: ssd_gauss_newton_composed).

Truth: autograd through `grid_pull(..., displacement=True)` for the gradient, `grid_grad` for the Hessian, the dense solve of
tests/test_regulariser_solve_cpu.py for the layout of the full Hessian -- never the function under test.

The device test (tests/test_ssd_gpu.py) shares `problem`, `nudged`, `reference` and `ratio` below: its reference is this
composed form in float64 on the CPU, at the coordinates the kernel forms in its own precision.
"""
import itertools

import pytest
import torch

import interpol
from interpol import ops
from interpol.codes import order_to_code
import test_regulariser_cpu as truth
import test_regulariser_solve_cpu as st

BOUNDS = ["zero", "replicate", "dct1", "dct2", "dst1", "dst2", "dft"]
ORDERS = [1, 2, 3]
# (inshape of `moving`, shape of `fixed` / `disp`)
CPU_SHAPES = [((7,), (5,)), ((5, 7), (4, 7)), ((4, 5, 6), (3, 5, 4)), ((1, 2, 3), (2, 1, 3))]
IDS = lambda shapes: ["%s-%s" % ("x".join(map(str, a)), "x".join(map(str, b))) for a, b in shapes]


def problem(inshape, shape, seed, dtype=torch.float64, C=3, B=2, sigma=2.0, weighted=True):
    """moving (B, C, *inshape), fixed (C, *shape) -- no batch: broadcast --, disp (B, *shape, D) = sigma N(0, 1), weight
    (B, *shape) in [0.5, 1.5) or None; drawn in float64 and rounded to `dtype` once"""
    gen = torch.Generator().manual_seed(seed)
    dim = len(shape)
    moving = torch.randn([B, C, *inshape], generator=gen, dtype=torch.float64)
    fixed = torch.randn([C, *shape], generator=gen, dtype=torch.float64)
    disp = sigma * torch.randn([B, *shape, dim], generator=gen, dtype=torch.float64)
    weight = 0.5 + torch.rand([B, *shape], generator=gen, dtype=torch.float64)
    return moving.to(dtype), fixed.to(dtype), disp.to(dtype), (weight.to(dtype) if weighted else None)


def lattice(shape, dtype):
    return torch.stack(torch.meshgrid(*[torch.arange(n, dtype=dtype) for n in shape], indexing="ij"), -1)


def nudged(disp, order):
    """`disp` with every coordinate o + disp (formed in the dtype of `disp`) that lies within 1e-3 of a spline knot (the integers
    for odd orders, the half-integers for order 2) or of a half-integer moved by 2^-7, repeatedly, until none is left; and the
    fraction of coordinates that were moved."""
    disp = disp.clone()
    o = lattice(disp.shape[-disp.shape[-1] - 1:-1], disp.dtype)
    moved = torch.zeros(disp.shape, dtype=torch.bool)

    def near(d):
        x = (o + d).double()
        half = (x - 0.5 - torch.round(x - 0.5)).abs() < 1e-3
        if order % 2 == 1:
            half = half | ((x - torch.round(x)).abs() < 1e-3)
        return half

    for _ in range(8):
        n = near(disp)
        if not bool(n.any()):
            break
        moved |= n
        disp[n] += 2.0 ** -7
    assert not bool(near(disp).any())
    return disp, float(moved.double().mean())


def in_view(disp, inshape):
    """fraction of the samples that `extrapolate=False` keeps: every coordinate in (-0.05, n - 1 + 0.05)"""
    x = (lattice(disp.shape[-disp.shape[-1] - 1:-1], disp.dtype) + disp).double()
    ok = torch.ones(x.shape[:-1], dtype=torch.bool)
    for d, n in enumerate(inshape):
        ok &= (x[..., d] > -0.05) & (x[..., d] < n - 1 + 0.05)
    return float(ok.double().mean())


def reference(moving, fixed, disp, weight, **kw):
    """the composed form on the CPU in float64, at the coordinates o + disp formed in the precision of `disp` and then widened"""
    o = lattice(disp.shape[-disp.shape[-1] - 1:-1], disp.dtype)
    x = (o + disp).double()                                              # what the kernel forms
    d64 = x - o.double()                                                 # exact in double: o + d64 == x
    assert torch.equal(o.double() + d64, x)
    w64 = None if weight is None else weight.double()
    return interpol.ssd_gauss_newton(moving.double(), fixed.double(), d64, w64, **kw)


def ratio(got, want, tol, scale):
    """max |got - want| / (tol scale + tol |want|)"""
    got, want = got.detach().cpu().double(), want.double()
    return float(((got - want).abs() / (tol * scale + tol * want.abs())).max()) if want.numel() else 0.0


def scales(moving, fixed, weight):
    """the natural scales of gradient and Hessian: (max|moving| + max|fixed|) max|moving| max weight, max|moving|^2 max weight"""
    m, f = float(moving.double().abs().max()), float(fixed.double().abs().max())
    w = 1.0 if weight is None else float(weight.double().abs().max())
    return (m + f) * m * w, m * m * w


# ---------------------------------------------------------------------------------------------------------------------
# 1. the gradient is d loss / d disp
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(CPU_SHAPES)), ids=IDS(CPU_SHAPES))
def test_gradient_is_autograd_of_the_loss(case):
    inshape, shape = CPU_SHAPES[case]
    worst = 0.0
    for n, (order, bound, extrapolate) in enumerate(itertools.product(ORDERS, BOUNDS, (False, True))):
        moving, fixed, disp, weight = problem(inshape, shape, 100 * case + n, weighted=n % 3 != 0)
        kw = dict(interpolation=order, bound=bound, extrapolate=extrapolate)
        loss, gradient, _ = interpol.ssd_gauss_newton(moving, fixed, disp, weight, hessian=None, **kw)
        u = disp.clone().requires_grad_()
        r = interpol.grid_pull(moving, u, displacement=True, **kw) - fixed
        w = 1.0 if weight is None else weight.unsqueeze(1)
        total = 0.5 * (w * r ** 2).sum()
        want, = torch.autograd.grad(total, u)
        assert loss.shape == (2,) and gradient.shape == disp.shape and gradient.dtype == torch.float64
        torch.testing.assert_close(loss.sum(), total.detach(), rtol=1e-12, atol=0)
        den = float(want.abs().max())
        if den:
            worst = max(worst, float((gradient - want).abs().max()) / den)
        torch.testing.assert_close(gradient, want, rtol=1e-12, atol=0, msg=lambda m: "%s %s: %s" % (shape, kw, m))
    print("gradient against autograd %s -> %s: largest relative difference %.3g" % (inshape, shape, worst))


# ---------------------------------------------------------------------------------------------------------------------
# 2. the Hessian
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(CPU_SHAPES)), ids=IDS(CPU_SHAPES))
def test_hessian_is_the_sum_of_outer_products_of_grid_grad(case):
    inshape, shape = CPU_SHAPES[case]
    dim = len(shape)
    for n, (order, bound, extrapolate) in enumerate(((1, "dct2", True), (2, "zero", False), (3, "dft", True), (3, "dst1", False))):
        moving, fixed, disp, weight = problem(inshape, shape, 700 + 10 * case + n, weighted=n % 2 == 0)
        kw = dict(interpolation=order, bound=bound, extrapolate=extrapolate)
        G = interpol.grid_grad(moving, disp, displacement=True, **kw)                            # (B, C, *shape, D)
        want = st.pack(torch.einsum("bc...d,bc...e->b...de", G, G))
        if weight is not None:
            want = want * weight.unsqueeze(-1)
        loss, gradient, full = interpol.ssd_gauss_newton(moving, fixed, disp, weight, hessian="full", **kw)
        assert full.shape == (2, *shape, dim * (dim + 1) // 2)
        torch.testing.assert_close(full, want, rtol=1e-12, atol=1e-14)
        l1, g1, diag = interpol.ssd_gauss_newton(moving, fixed, disp, weight, hessian="diagonal", **kw)
        assert diag.shape == (2, *shape, dim) and torch.equal(diag, full[..., :dim])
        l0, g0, none = interpol.ssd_gauss_newton(moving, fixed, disp, weight, hessian=None, **kw)
        assert none is None
        for l, g in ((l1, g1), (l0, g0)):
            assert torch.equal(l, loss) and torch.equal(g, gradient)


@pytest.mark.parametrize("shape", [(9,), (4, 3)], ids=["9", "4x3"])
def test_full_hessian_is_the_layout_regulariser_solve_takes(shape):
    """(H + L) x = g with the H of ssd_gauss_newton against torch.linalg.solve of the assembled matrix"""
    dim = len(shape)
    moving, fixed, disp, weight = problem(tuple(n + 2 for n in shape), shape, 31 + dim, C=2, sigma=0.7)
    loss, g, h = interpol.ssd_gauss_newton(moving, fixed, disp, weight, interpolation=3, bound="dct2", hessian="full")
    w = dict(absolute=0.05, membrane=0.8)
    got = interpol.regulariser_solve(g, h, bound="dct2", max_iter=400, **w)
    S = truth.spatial_matrix(shape, "dct2", **w)
    Hd = st.unpack(h, dim)
    for b in range(2):
        A = st.dense_matrix(S, truth.h2(dim), Hd[b].reshape(-1, dim, dim))
        want = torch.linalg.solve(A, g[b].reshape(-1)).reshape(g[b].shape)
        assert float((got[b] - want).abs().max()) <= 1e-9 * float(want.abs().max()), (shape, b)


# ---------------------------------------------------------------------------------------------------------------------
# 3. one Gauss-Newton step lowers the objective
# ---------------------------------------------------------------------------------------------------------------------
def blobs(n, dim, dtype, device="cpu"):
    """a Gaussian blob and the same blob shifted by a voxel or so: (1, *[n] * dim) each"""
    x = lattice([n] * dim, torch.float64)
    c = (n - 1) / 2
    shift = torch.tensor([1.0, -0.6, 0.8][:dim], dtype=torch.float64)
    blob = lambda centre: torch.exp(-((x - centre) ** 2).sum(-1) / (2 * (n / 6) ** 2))[None]
    return blob(c).to(dtype).to(device), blob(c + shift).to(dtype).to(device)


def gauss_newton_step(moving, fixed, disp, membrane=0.5):
    """-> (objective before, objective after) of one step disp - (H + L)^-1 (g + L disp)"""
    kw = dict(interpolation=3, bound="dct2", extrapolate=True)
    reg = dict(membrane=membrane, bound="dct2")
    loss, g, h = interpol.ssd_gauss_newton(moving, fixed, disp, hessian="full", **kw)
    before = loss + interpol.regulariser_energy(disp, **reg)
    x = interpol.regulariser_solve(g + interpol.regulariser(disp, **reg), h, max_iter=16, **reg)
    new = disp - x
    after = interpol.ssd_gauss_newton(moving, fixed, new, hessian=None, **kw)[0] + interpol.regulariser_energy(new, **reg)
    return before, after


def test_one_gauss_newton_step_lowers_the_objective():
    moving, fixed = blobs(16, 2, torch.float64)
    disp = torch.zeros(16, 16, 2, dtype=torch.float64)
    before, after = gauss_newton_step(moving, fixed, disp)
    print("objective %.6g -> %.6g" % (float(before), float(after)))
    assert float(before) > 0 and float(after) < 0.5 * float(before)


# ---------------------------------------------------------------------------------------------------------------------
# 4. arguments
# ---------------------------------------------------------------------------------------------------------------------
def test_batch_broadcasting_copies_nothing(monkeypatch):
    inshape, shape = (4, 5, 6), (3, 5, 4)
    moving, fixed, disp, weight = problem(inshape, shape, 900)
    kw = dict(interpolation=2, bound="dct1", extrapolate=False)
    seen = []
    fn = ops.ssd_gauss_newton

    def spy(m, f, u, w, *a):
        seen.append((m, f, u, w))
        return fn(m, f, u, w, *a)

    monkeypatch.setattr(ops, "ssd_gauss_newton", spy)
    loss, g, h = interpol.ssd_gauss_newton(moving, fixed, disp, weight, **kw)                    # fixed without a batch
    m, f, u, w = seen[-1]
    assert f.shape == (1, 3, *shape) and f.data_ptr() == fixed.data_ptr() and m.data_ptr() == moving.data_ptr()
    assert u.data_ptr() == disp.data_ptr() and w.data_ptr() == weight.data_ptr()
    le, ge, he = interpol.ssd_gauss_newton(moving, fixed.expand(2, *fixed.shape).contiguous(), disp, weight, **kw)
    assert torch.equal(loss, le) and torch.equal(g, ge) and torch.equal(h, he)
    # a stride-0 batch is not materialised either
    ls, gs, hs = interpol.ssd_gauss_newton(moving, fixed[None].expand(2, *fixed.shape), disp, weight[:1].expand_as(weight), **kw)
    m, f, u, w = seen[-1]
    assert f.stride(0) == 0 and f.data_ptr() == fixed.data_ptr() and w.stride(0) == 0 and w.data_ptr() == weight.data_ptr()
    l1, g1, h1 = interpol.ssd_gauss_newton(moving, fixed, disp, weight[:1].expand_as(weight).contiguous(), **kw)
    assert torch.equal(ls, l1) and torch.equal(gs, g1) and torch.equal(hs, h1)
    # only `moving` has a batch: the others serve every item
    l2, g2, h2 = interpol.ssd_gauss_newton(moving, fixed, disp[0], weight[0], **kw)
    m, f, u, w = seen[-1]
    assert u.shape[0] == 1 and w.shape[0] == 1 and u.data_ptr() == disp.data_ptr()
    assert l2.shape == (2,) and g2.shape == disp.shape and h2.shape == h.shape
    assert torch.equal(l2[0], loss[0]) and torch.equal(g2[0], g[0]) and torch.equal(h2[0], h[0])
    # leading batch dimensions fold; no batch at all gives a scalar loss
    l3, g3, h3 = interpol.ssd_gauss_newton(moving.reshape(2, 1, *moving.shape[1:]), fixed, disp.reshape(2, 1, *disp.shape[1:]),
                                           weight, **kw)
    assert l3.shape == (2, 2) and g3.shape == (2, 2, *shape, 3) and h3.shape == (2, 2, *shape, 6)
    assert torch.equal(l3[0, 0], loss[0]) and torch.equal(g3[1, 1], g[1])
    l4, g4, h4 = interpol.ssd_gauss_newton(moving[0], fixed, disp[0], weight[0], **kw)
    assert l4.shape == () and g4.shape == disp[0].shape and torch.equal(g4, g[0]) and torch.equal(l4, loss[0])
    # only `weight` has a batch -- as it comes, and with the other operands as explicit batches of 1
    for kind in ("full", "diagonal", None):
        l5, g5, h5 = interpol.ssd_gauss_newton(moving[0], fixed, disp[0], weight, hessian=kind, **dict(kw))
        l6, g6, h6 = interpol.ssd_gauss_newton(moving[:1], fixed[None], disp[:1], weight, hessian=kind, **dict(kw))
        assert l5.shape == (2,) and g5.shape == disp.shape and (h5 is None) == (kind is None)
        assert torch.equal(l5, l6) and torch.equal(g5, g6) and (kind is None or torch.equal(h5, h6))
        for b in range(2):
            lb, gb, hb = interpol.ssd_gauss_newton(moving[0], fixed, disp[0], weight[b], hessian=kind, **dict(kw))
            torch.testing.assert_close(l5[b], lb, rtol=1e-12, atol=0)
            assert torch.equal(g5[b], gb)
            if kind is not None:
                assert h5.shape == (2, *shape, 6 if kind == "full" else 3) and torch.equal(h5[b], hb)


def test_weight_scales_the_three_outputs():
    moving, fixed, disp, weight = problem((5, 7), (4, 7), 910)
    kw = dict(interpolation=3, bound="replicate", extrapolate=True)
    l1, g1, h1 = interpol.ssd_gauss_newton(moving, fixed, disp, None, **kw)
    lo, go, ho = interpol.ssd_gauss_newton(moving, fixed, disp, torch.ones_like(weight), **kw)
    assert torch.equal(l1, lo) and torch.equal(g1, go) and torch.equal(h1, ho)
    lw, gw, hw = interpol.ssd_gauss_newton(moving, fixed, disp, weight, **kw)
    torch.testing.assert_close(gw, g1 * weight.unsqueeze(-1), rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(hw, h1 * weight.unsqueeze(-1), rtol=1e-12, atol=1e-14)
    r = interpol.grid_pull(moving, disp, displacement=True, **kw) - fixed
    torch.testing.assert_close(lw, 0.5 * (weight.unsqueeze(1) * r ** 2).sum([1, 2, 3]), rtol=1e-12, atol=0)
    # a zero weight switches a voxel off
    weight[:, 1, 2] = 0
    lz, gz, hz = interpol.ssd_gauss_newton(moving, fixed, disp, weight, **kw)
    assert not bool(gz[:, 1, 2].any()) and not bool(hz[:, 1, 2].any()) and bool(gz[:, 1, 3].any())


def test_prefilter_is_spline_coeff_nd_first():
    moving, fixed, disp, weight = problem((4, 5, 6), (3, 5, 4), 920)
    for order in (1, 3, [1, 2, 3]):
        kw = dict(interpolation=order, bound="dct2", extrapolate=True)
        got = interpol.ssd_gauss_newton(moving, fixed, disp, weight, prefilter=True, **kw)
        coeff = interpol.spline_coeff_nd(moving, interpolation=order, bound="dct2", dim=3)
        want = interpol.ssd_gauss_newton(coeff, fixed, disp, weight, **kw)
        plain = interpol.ssd_gauss_newton(moving, fixed, disp, weight, **kw)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
        assert torch.equal(got[1], plain[1]) == (order == 1)             # orders 0 and 1 have nothing to filter


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_sixteen_bit_inputs_compute_in_float32_and_round_once(dtype):
    moving, fixed, disp, weight = problem((4, 5, 6), (3, 5, 4), 930, dtype=dtype, sigma=0.7)
    kw = dict(interpolation=3, bound="dct2", extrapolate=True)
    got = interpol.ssd_gauss_newton(moving, fixed, disp, weight, **kw)
    want = interpol.ssd_gauss_newton(moving.float(), fixed.float(), disp.float(), weight.float(), **kw)
    for a, b in zip(got, want):
        assert a.dtype == dtype and b.dtype == torch.float32 and torch.equal(a, b.to(dtype))


def test_four_dimensions_and_aliases():
    inshape, shape = (3, 2, 4, 3), (2, 3, 3, 2)
    moving, fixed, disp, weight = problem(inshape, shape, 940, C=2, sigma=0.8)
    kw = dict(interpolation=["linear", 2, "cubic", 1], bound=["mirror", "dct2", "circular", "zero"], extrapolate=False)
    loss, g, h = interpol.ssd_gauss_newton(moving, fixed, disp, weight, **kw)
    assert loss.shape == (2,) and g.shape == (2, *shape, 4) and h.shape == (2, *shape, 10)
    u = disp.clone().requires_grad_()
    r = interpol.grid_pull(moving, u, displacement=True, **kw) - fixed
    want, = torch.autograd.grad(0.5 * (weight.unsqueeze(1) * r ** 2).sum(), u)
    torch.testing.assert_close(g, want, rtol=1e-12, atol=0)
    G = interpol.grid_grad(moving, disp, displacement=True, **kw)
    torch.testing.assert_close(h, st.pack(torch.einsum("bc...d,bc...e->b...de", G, G)) * weight.unsqueeze(-1), rtol=1e-12, atol=1e-14)
    assert order_to_code("cubic") == 3


def test_argument_errors():
    moving, fixed, disp, weight = problem((4, 5, 6), (3, 5, 4), 950)
    ok = dict(interpolation=1, bound="dct2")
    with pytest.raises(ValueError, match="dtype and device"):
        interpol.ssd_gauss_newton(moving.float(), fixed, disp, weight, **ok)
    with pytest.raises(ValueError, match="dtype and device"):
        interpol.ssd_gauss_newton(moving, fixed, disp, weight.float(), **ok)
    with pytest.raises(ValueError, match="dtype and device"):
        interpol.ssd_gauss_newton(moving, fixed.to("meta"), disp, weight, **ok)
    with pytest.raises(ValueError, match="floating point"):
        interpol.ssd_gauss_newton(moving, fixed.long(), disp, weight, **ok)
    with pytest.raises(ValueError, match="channels"):
        interpol.ssd_gauss_newton(moving[:, :2], fixed, disp, weight, **ok)
    with pytest.raises(ValueError, match="spatial shape"):
        interpol.ssd_gauss_newton(moving, fixed[..., :3], disp, weight, **ok)
    with pytest.raises(ValueError, match="spatial shape"):
        interpol.ssd_gauss_newton(moving, fixed, disp[:, :2], weight, **ok)
    with pytest.raises(ValueError, match="spatial shape"):
        interpol.ssd_gauss_newton(moving, fixed, disp, weight[..., :3], **ok)
    with pytest.raises(ValueError, match="number of spatial dimensions"):
        interpol.ssd_gauss_newton(moving[0, 0], fixed[0], disp[0], None, **ok)            # (*inshape) without a channel
    with pytest.raises(ValueError, match="number of spatial dimensions"):
        interpol.ssd_gauss_newton(moving, fixed, torch.zeros(5, 4, 7, dtype=torch.float64), None, **ok)   # D = 7, two spatial dims
    for bad in ("upper", "diag", 6, True):
        with pytest.raises(ValueError, match="hessian"):
            interpol.ssd_gauss_newton(moving, fixed, disp, weight, hessian=bad, **ok)
    for name in ("moving", "fixed", "disp", "weight"):
        args = dict(moving=moving, fixed=fixed, disp=disp, weight=weight)
        args[name] = args[name].clone().requires_grad_()
        with pytest.raises(RuntimeError, match="not differentiable"):
            interpol.ssd_gauss_newton(**args, **ok)
        with torch.no_grad():
            out = interpol.ssd_gauss_newton(**args, **ok)
        assert not any(t.requires_grad for t in out)
        out = interpol.ssd_gauss_newton(**{k: v.detach() for k, v in args.items()}, **ok)
        assert not any(t.requires_grad for t in out)
