"""`interpol.mi_gauss_newton` on the device (csrc/mi.hip).

Truth: the composed form in float64 on the CPU, fed the upcast inputs (tests/test_mi_cpu.py: `truth_and_allowance`).  The
displacements are dyadic (multiples of 1/32: i.i.d. normal of sigma = 2 rounded, a smooth one, and the smooth one shifted so that
part of the lattice leaves the view), so o + disp is exact in float32: both sides see the same `floor` and the same mask.  The fixed
images hold k + delta with integer k and dyadic |delta| <= 1/4 under an explicit fixed_range = (0, B - 1): no sample sits near a bin
edge, the float32 and the float64 side pick the same bin.

Allowance (derived in `truth_and_allowance` there): tol = 1e-5 (float32) / 1e-11 (float64) times A = 1 + (B - 4) max|moving| m_sc;
the loss and P as tests/test_mi_affine_gpu.py; the two fields per sample, tol A (|q_d(o)| + max_o |q_d|) + dT q0_d(o) and the
same with h and h0, plus the quantum of the fixed-point histogram as T = log P carries it into a sample (a correction derived there
from the number format; it matters where a bin is nearly empty), at every sample whose t_m is not within 4 tol max|moving| m_sc of its
clamp (at most max(1, N / 1000) per item are left out, asserted from the truth alone).

Lattices (moving -> fixed), each for a way the kernels can go wrong: 1x1x1 and 2x1x1 leave all but one workgroup without a sample;
5x6x7 is six partial 4 x 2 x 32 boxes; 9x33x70 has odd y and z with a partial box; 40x96x72 has 276 480 samples, more than 512 * 256,
so every histogram workgroup loops; 33x70 and 600x450, 7 and 300 000 are their 2-D and 1-D counterparts.
"""
import ctypes

import pytest
import torch

import interpol
from interpol import _hip, backend, ops, torch_kernels
from interpol.sepgrid import AffineGrid
import memguard
import test_mi_affine_cpu as aff
import test_mi_cpu as cpu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = {torch.float32: 1e-5, torch.float64: 1e-11}
F32, F64 = torch.float32, torch.float64
ALL_ORDERS = (1, 2, 3)

# (moving, fixed lattice, dtype, order, bound, extrapolate, bins, weighted, hessian, moving_range, field)
PARITY = [
    ((3, 2, 2), (1, 1, 1), F64, 1, "dct2", True, 8, False, "full", None, "noise"),
    ((3, 2, 2), (2, 1, 1), F32, 2, "dft", True, 32, True, "full", None, "smooth"),
    ((7, 5, 6), (5, 6, 7), F64, 3, "zero", False, 8, True, "diagonal", None, "shifted"),
    ((7, 5, 6), (5, 6, 7), F32, 1, "replicate", 2, 64, False, None, (-1.0, 1.5), "noise"),
    ((12, 30, 64), (9, 33, 70), F64, 2, "replicate", 2, 32, True, "full", (-1.0, 1.5), "smooth"),
    ((44, 90, 80), (40, 96, 72), F32, 3, "dct2", True, 32, True, "full", None, "noise"),
    ((44, 90, 80), (40, 96, 72), F64, 1, "dft", False, 64, False, "diagonal", None, "shifted"),
    ((40, 64), (33, 70), F64, 3, "dft", False, 8, True, None, None, "shifted"),
    ((40, 64), (33, 70), F32, 2, "zero", True, 32, False, "full", None, "noise"),
    ((512, 512), (600, 450), F32, 1, "dct2", False, 64, True, "full", None, "shifted"),
    ((512, 512), (600, 450), F64, 2, "zero", 2, 32, False, "diagonal", (-2.0, 2.0), "smooth"),
    ((9,), (7,), F64, 3, "replicate", True, 8, True, "full", None, "noise"),
    ((270000,), (300000,), F32, 2, "dct2", True, 64, False, "full", None, "noise"),
    ((250000,), (300000,), F64, 1, "zero", False, 32, True, "full", None, "shifted"),
]


def case_id(c):
    return "%s-%s-o%d-%s-e%d-B%d%s-%s%s-%s" % ("x".join(map(str, c[1])), "f32" if c[2] == F32 else "f64", c[3], c[4], int(c[5]), c[6],
                                               "-w" if c[7] else "", c[8] or "nohess", "-range" if c[9] else "", c[10])


def field(kind, shape, dtype, seed, lead=()):
    """a dyadic displacement (lead..., *shape, D): "noise" i.i.d. normal of sigma = 2, "smooth", "shifted" = smooth + 2.5"""
    dim = len(shape)
    if kind == "noise":
        return cpu.dyadic_noise(shape, dim, torch.Generator().manual_seed(seed), 2.0, lead).to(dtype)
    d = cpu.dyadic_smooth(shape, dim, 1.5, 2.5 if kind == "shifted" else 0.0)
    return d.expand(*lead, *d.shape).contiguous().to(dtype)


def fused_calls(monkeypatch):
    """count the calls that reach the binding of the library"""
    calls = dict(n=0)
    fn = _hip.mi

    def f(*a, **k):
        calls["n"] += 1
        return fn(*a, **k)

    monkeypatch.setattr(_hip, "mi", f)
    return calls


def route_all(monkeypatch):
    monkeypatch.setattr(backend, "fused_mi_orders", ALL_ORDERS)


def dev(t):
    return None if t is None else t.to(DEV)


def same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


def no_sample_near_a_bin_edge(fixed, bins):
    t = fixed.double()
    return bool(((t - t.round()).abs() <= 0.25 + 1e-9).all()) and bool((fixed >= 0).all()) and bool((fixed <= bins - 1).all())


def check(got, want, allow, keep, what, hessian="full"):
    ratios = dict(loss=aff.worst_ratio(got[0], want[0], allow[0]), gradient=cpu.worst_field_ratio(got[1], want[1], allow[1], keep),
                  P=aff.worst_ratio(got[3], want[3], allow[3]))
    if hessian is not None:
        ratios["hessian"] = cpu.worst_field_ratio(got[2], want[2], allow[2], keep)
    else:
        assert got[2] is None, what
    print("parity %s: worst error / allowance: %s; left out %d of %d samples"
          % (what, ", ".join("%s %.3g" % kv for kv in ratios.items()), int((~keep).sum()), keep.numel()))
    assert all(v <= 1.0 for v in ratios.values()), (what, ratios)
    return ratios


# ---------------------------------------------------------------------------------------------------------------------
# 1. parity with the composed form in float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PARITY, ids=case_id)
def test_parity_with_the_composed_form_in_float64(case, monkeypatch):
    inshape, shape, dtype, order, bound, extrapolate, bins, weighted, hessian, mrange, kind = case
    route_all(monkeypatch)
    calls = fused_calls(monkeypatch)
    dim = len(shape)
    seed = 2000 + PARITY.index(case)
    moving, fixed, weight = aff.problem(inshape, shape, seed, dtype, bins=bins, B=1, weighted=weighted)
    assert no_sample_near_a_bin_edge(fixed, bins)
    disp = field(kind, shape, dtype, seed, (1,))
    kw = dict(interpolation=order, bound=bound, extrapolate=extrapolate)
    mi = dict(bins=bins, moving_range=mrange, fixed_range=(0, bins - 1))
    want, allow, keep = cpu.truth_and_allowance(moving, fixed, disp, weight, TOL[dtype], hessian=hessian, **mi, **kw)
    if kind == "shifted" and extrapolate is False:                       # part of the lattice is out of view, part of it in view
        x = disp[0].double() + interpol.identity_grid(shape, dtype=torch.float64)
        inside = torch_kernels._mask(x, inshape, 0).double().mean()
        assert 0.0 < float(inside) < 1.0, float(inside)
    got = interpol.mi_gauss_newton(dev(moving), dev(fixed), dev(disp), dev(weight), hessian=hessian, return_histogram=True, **mi, **kw)
    assert calls["n"] == 1
    K = {None: 0, "diagonal": dim, "full": dim * (dim + 1) // 2}[hessian]
    assert got[0].shape == (1,) and got[1].shape == (1, *shape, dim) and (not K or got[2].shape == (1, *shape, K))
    assert got[3].shape == (1, bins, bins)
    assert all(t.dtype == dtype and t.is_cuda for t in got if t is not None)
    check(got, want, allow, keep, case_id(case), hessian)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_a_batch_with_a_shared_moving_image_and_a_batched_weight(dtype, monkeypatch):
    route_all(monkeypatch)
    calls = fused_calls(monkeypatch)
    bins, shape = 8, (5, 6, 7)
    moving, fixed, weight = aff.problem((7, 5, 6), shape, 2100, dtype, bins=bins, B=3)
    disp = field("noise", shape, dtype, 2101, (3,))
    disp[1] = field("smooth", shape, dtype, 0)
    kw = dict(interpolation=2, bound="dct2", extrapolate=False)
    mi = dict(bins=bins, moving_range=None, fixed_range=(0, bins - 1))
    for m, f, u, w in ((moving[:1], fixed, disp, weight), (moving[:1], fixed[:1], disp[:1], weight), (moving, fixed[:1], disp, None)):
        want, allow, keep = cpu.truth_and_allowance(m, f, u, w, TOL[dtype], **mi, **kw)
        got = interpol.mi_gauss_newton(dev(m), dev(f), dev(u), dev(w), return_histogram=True, **mi, **kw)
        assert got[0].shape == (3,) and got[1].shape == (3, *shape, 3) and got[2].shape == (3, *shape, 6) and got[3].shape == (3, bins, bins)
        check(got, want, allow, keep, "B=3 %s moving %d fixed %d disp %d weight %s" % (dtype, m.shape[0], f.shape[0], u.shape[0], w is not None))
    assert calls["n"] == 3


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_the_fused_affine_and_the_fused_dense_term_agree(dtype, monkeypatch):
    """On the dense field of a dyadic matrix (exact in float32) both histograms and both losses lie within their allowances of one
    truth; whether they are bit-identical is printed, not asserted (the two histogram kernels form the coordinate differently)."""
    route_all(monkeypatch)
    monkeypatch.setattr(backend, "fused_mi_affine_orders", ALL_ORDERS)
    bins, inshape, shape = 32, (12, 30, 64), (9, 33, 70)
    moving, fixed, weight = aff.problem(inshape, shape, 2200, dtype, bins=bins, B=1)
    mat = aff.matrix(3, dtype)[None]
    disp = (AffineGrid(mat[0].double(), shape).dense().reshape(1, *shape, 3) - interpol.identity_grid(shape, dtype=torch.float64)).to(dtype)
    assert torch.equal(disp.double() + interpol.identity_grid(shape, dtype=torch.float64), AffineGrid(mat[0].double(), shape).dense().reshape(1, *shape, 3))
    kw = dict(interpolation=3, bound="dct2", extrapolate=False)
    mi = dict(bins=bins, moving_range=None, fixed_range=(0, bins - 1))
    want, allow = aff.truth_and_allowance(moving, fixed, mat, weight, TOL[dtype], **mi, **kw)
    a = interpol.mi_gauss_newton_affine(dev(moving), dev(fixed), dev(mat), dev(weight), return_histogram=True, **mi, **kw)
    d = interpol.mi_gauss_newton(dev(moving), dev(fixed), dev(disp), dev(weight), return_histogram=True, **mi, **kw)
    for name, got in (("affine", a), ("dense", d)):
        ratios = dict(loss=aff.worst_ratio(got[0], want[0], allow[0]), P=aff.worst_ratio(got[3], want[3], allow[3]))
        print("fused %s %s against the affine truth: worst error / allowance: %s" % (name, dtype, ratios))
        assert all(v <= 1.0 for v in ratios.values()), (name, ratios)
    print("fused affine and fused dense %s: histogram bit-identical %s, loss bit-identical %s"
          % (dtype, torch.equal(a[3], d[3]), torch.equal(a[0], d[0])))


# ---------------------------------------------------------------------------------------------------------------------
# 2. routing
# ---------------------------------------------------------------------------------------------------------------------
def test_default_routing_reaches_the_fused_kernels_once(monkeypatch):
    calls = fused_calls(monkeypatch)
    assert isinstance(backend.fused_mi_orders, tuple) and set(backend.fused_mi_orders) <= set(ALL_ORDERS)
    for (inshape, shape), dtype in ((((7, 5, 6), (5, 6, 7)), F32), (((40, 64), (33, 70)), F64), (((9,), (7,)), F32)):
        dim = len(shape)
        moving, fixed, weight = (dev(t) for t in aff.problem(inshape, shape, 2300, dtype, B=2))
        disp = dev(field("smooth", shape, dtype, 0))
        for order in ALL_ORDERS:
            routed = order in backend.fused_mi_orders
            assert ops.mi_covered(moving, fixed, disp[None], weight, [order], 32) == routed
            before = calls["n"]
            loss, g, h = interpol.mi_gauss_newton(moving, fixed, disp, weight, interpolation=order)
            assert calls["n"] - before == routed
            assert loss.shape == (2,) and g.shape == (2, *shape, dim) and h.shape == (2, *shape, dim * (dim + 1) // 2)
            assert all(t.dtype == dtype and t.is_cuda for t in (loss, g, h))


@pytest.mark.parametrize("what", ["bf16", "4d", "mixed_orders", "many_bins", "switched_off"])
def test_uncovered_classes_take_the_composed_route(what, monkeypatch):
    """Each case differs from a call that reaches the fused kernels in ONE property; the control is asserted to reach the binding."""
    route_all(monkeypatch)
    calls = fused_calls(monkeypatch)
    control = [dev(t) for t in aff.problem((7, 5, 6), (5, 6, 7), 2400, F32)]
    cdisp = dev(field("smooth", (5, 6, 7), F32, 0))
    interpol.mi_gauss_newton(control[0], control[1], cdisp, control[2], interpolation=1, bins=8)
    assert calls["n"] == 1
    order = [1, 2, 3] if what == "mixed_orders" else 1
    bins = 65 if what == "many_bins" else 8
    if what == "4d":
        gen = torch.Generator().manual_seed(5)
        moving, fixed, weight = torch.randn(2, 1, 4, 3, 4, 3, generator=gen), aff.binned((3, 4, 3, 2), 8, gen, [2, 1]).float(), None
        disp = cpu.dyadic_noise((3, 4, 3, 2), 4, gen, 0.5).float()
    else:
        moving, fixed, weight = aff.problem((7, 5, 6), (5, 6, 7), 2400, torch.bfloat16 if what == "bf16" else F32)
        disp = field("smooth", (5, 6, 7), moving.dtype, 0)
    if what == "switched_off":
        monkeypatch.setattr(backend, "fused_mi_orders", ())
    kw = dict(interpolation=order, bound="dct2", extrapolate=True, bins=bins)
    got = interpol.mi_gauss_newton(dev(moving), dev(fixed), dev(disp), dev(weight), **kw)
    assert calls["n"] == 1 and all(t.dtype == moving.dtype and t.is_cuda for t in got)
    want = interpol.mi_gauss_newton(moving.double(), fixed.double(), disp.double(), None if weight is None else weight.double(), **kw)
    tol = 2e-2 if what == "bf16" else 1e-4                                 # relative to the largest entry: the composed route in float32
    for g, w in zip(got, want):
        assert float((g.double().cpu() - w).abs().max()) <= tol * float(w.abs().max()), what


def test_two_channels_raise():
    moving, fixed, _ = aff.problem((7, 5, 6), (5, 6, 7), 2500, F32)
    with pytest.raises(ValueError, match="ONE channel"):
        interpol.mi_gauss_newton(dev(moving.expand(2, 7, 5, 6)), dev(fixed.expand(2, 5, 6, 7)), dev(field("smooth", (5, 6, 7), F32, 0)))


# ---------------------------------------------------------------------------------------------------------------------
# 3. bits
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_bits_do_not_depend_on_the_run_or_on_the_batch(dtype, monkeypatch):
    route_all(monkeypatch)
    for inshape, shape, order, hessian, bins in (((7, 5, 6), (5, 6, 7), 3, "full", 8), ((12, 30, 64), (9, 33, 70), 1, "diagonal", 32),
                                                 ((40, 64), (33, 70), 2, None, 64), ((9,), (300,), 2, "full", 16)):
        moving, fixed, weight = (dev(t) for t in aff.problem(inshape, shape, 2600, dtype, bins=bins, B=3))
        disp = dev(field("noise", shape, dtype, 2601, (3,)))
        kw = dict(interpolation=order, bound="dct2", extrapolate=False, hessian=hessian, bins=bins, return_histogram=True)
        a = interpol.mi_gauss_newton(moving, fixed, disp, weight, **kw)
        b = interpol.mi_gauss_newton(moving, fixed, disp, weight, **kw)
        assert same(a, b), (shape, order)
        assert bool((a[0] <= 0).all()) and bool(a[1].isfinite().all()) and (hessian is None or bool(a[2].isfinite().all()))
        for i in (0, 2):
            one = interpol.mi_gauss_newton(moving[i], fixed[i], disp[i], weight[i], **kw)
            assert same(one, [None if t is None else t[i] for t in a]), (shape, order, i)


def test_graph_replay_gives_the_bits_of_eager(monkeypatch):
    route_all(monkeypatch)
    shape = (9, 33, 70)
    moving, fixed, weight = (dev(t) for t in aff.problem((12, 30, 64), shape, 2700, F32, bins=32, B=2))
    disp = dev(field("noise", shape, F32, 2701, (2,)))
    kw = dict(interpolation=3, bound="dct2", extrapolate=True, bins=32, return_histogram=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                        # warm-up on the side stream (module loads)
        interpol.mi_gauss_newton(moving, fixed, disp, weight, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = interpol.mi_gauss_newton(moving, fixed, disp, weight, **kw)
    for it in range(3):
        disp += 0.5 * (it + 1)
        graph.replay()
        torch.cuda.synchronize()
        eager = interpol.mi_gauss_newton(moving, fixed, disp, weight, **kw)
        assert same(out, eager), it
        assert bool(out[0].isfinite().all()) and bool((out[0] < 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# 4. memory contract
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("misalign", [0, 1, 3])
def test_memory_contract(misalign, dtype):
    """Three items: an ordinary one, one whose weight is zero (W = 0) and one whose field leaves the view altogether."""
    for inshape, shape, hessian, bins in (((7, 5, 6), (5, 6, 7), "full", 8), ((12, 30, 64), (9, 33, 70), "diagonal", 64),
                                          ((40, 64), (33, 70), None, 32), ((9,), (7,), "full", 9)):
        dim = len(shape)
        moving, fixed, weight = aff.problem(inshape, shape, 2800, dtype, bins=bins, B=3)
        weight[1] = 0
        disp = field("noise", shape, dtype, 2801, (3,))
        disp[2] += 1000.0
        args = [moving, fixed, disp, weight]
        ranges = torch_kernels.mi_ranges(dev(moving), dev(fixed), dev(weight), None, (0, bins - 1), 3)
        for bound, extrapolate in ((3, 1), (6, 0)):
            opt = ([bound] * 3, [3] * 3, extrapolate, hessian, bins, True)
            ref = _hip.mi(*[dev(t) for t in args], ranges, *opt)
            assert all(bool(torch.isfinite(r).all()) for r in ref if r is not None)
            assert all(bool((r[1] == 0).all()) for r in ref if r is not None)                     # W = 0: zeros
            if extrapolate == 0:
                assert all(bool((r[2] == 0).all()) for r in ref if r is not None)                 # out of view: zeros
            with memguard.installed(_hip, misalign=misalign) as seam:
                placed = [memguard.place(t, DEV, misalign=misalign) for t in args]
                out = _hip.mi(*placed, ranges, *opt)
                torch.cuda.synchronize()
                what = (shape, bound, misalign)
                assert len(seam.outputs()) == 3 + (hessian is not None) and len(seam.workspaces()) == 1 and seam.workspace_was_written(), what
                K = {None: 0, "diagonal": dim, "full": dim * (dim + 1) // 2}[hessian]
                assert out[0].shape == (3,) and out[1].shape == (3, *shape, dim) and (not K or out[2].shape == (3, *shape, K)), what
                assert out[3].shape == (3, bins, bins), what
                for t in [o for o in out if o is not None] + placed:
                    assert t.data_ptr() % memguard.ALIGN == misalign * t.element_size(), what
                for t, r in zip(out, ref):
                    if t is not None:
                        seam.assert_fully_written(t, r, what)
                        assert torch.equal(t, r), what
                seam.assert_guards_intact(what)
                for t, a in zip(placed, args):
                    memguard.assert_guard_intact(t, what)
                    assert torch.equal(t.cpu(), a), what


# ---------------------------------------------------------------------------------------------------------------------
# 5. the entry points validate before launching
# ---------------------------------------------------------------------------------------------------------------------
def raw_call(L, p, moving, fixed, disp, weight, ranges, loss, grad, hess, hist, kind, bins, wbs, gbs, hbs, ws, nbytes=None):
    ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)
    return L.interpol_mi(ctypes.byref(p), ptr(moving), ptr(fixed), ptr(disp), ptr(weight), ptr(ranges), ptr(loss), ptr(grad), ptr(hess),
                         ptr(hist), kind, bins, wbs, gbs, hbs, ptr(ws), (0 if ws is None else ws.numel()) if nbytes is None else nbytes,
                         ctypes.c_void_p(0))


def test_entry_points_validate_before_launching():
    L = _hip.lib()
    inshape, shape, bins = (6, 5, 4), (5, 4, 7), 16
    N = 5 * 4 * 7
    moving, fixed, weight = (dev(t) for t in aff.problem(inshape, shape, 2900, F32, bins=bins, B=2))
    disp = dev(field("noise", shape, F32, 2901, (2,)))
    ranges = torch_kernels.mi_ranges(moving, fixed, weight, None, (0, bins - 1), 2)
    sentinel = 4321.0
    loss = torch.full([2], sentinel, device=DEV)
    grad = torch.full([2, *shape, 3], sentinel, device=DEV)
    hess = torch.full([2, *shape, 6], sentinel, device=DEV)
    hist = torch.full([2, bins, bins], sentinel, device=DEV)

    def problem(dtype=F32, gdtype=None, dim=3, order=(3, 3, 3), bound=3, extrapolate=1, C=1, B=2, mstr=None, fstr=None, dstr=None,
                flags=0, inshp=inshape, shp=shape):
        m = mstr or [moving.stride(0), moving.stride(1), *moving.stride()[2:]]
        f = fstr or [fixed.stride(0), fixed.stride(1), *fixed.stride()[2:], 0, 0]
        d = dstr or [disp.stride(0), *disp.stride()[1:4], 1]
        return _hip.make_problem(dim, dtype, gdtype or dtype, [bound] * 3, list(order), extrapolate, B, C, inshp, shp, m, d, f, flags)

    need = L.interpol_mi_workspace(ctypes.byref(problem()), bins)
    assert need == 2 * (2 * bins * bins * 8 + 8)                         # two tables and 1 / W per item
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)

    def call(p, m=moving, f=fixed, u=disp, w=weight, r=ranges, lo=loss, g=grad, h=hess, hi=hist, kind=2, nb=bins, wbs=N, gbs=3 * N,
             hbs=6 * N, work=ws, nbytes=None):
        return raw_call(L, p, m, f, u, w, r, lo, g, h, hi, kind, nb, wbs, gbs, hbs, work, nbytes)

    for dim in (0, 4):
        assert call(problem(dim=dim)) == -1                             # INTERPOL_E_DIM
    for order in ((0, 0, 0), (4, 4, 4), (1, 2, 3)):
        assert call(problem(order=order)) == -2                         # INTERPOL_E_ORDER: one order 1..3
    assert call(problem(bound=7)) == -3                                 # INTERPOL_E_BOUND
    assert call(problem(dtype=torch.bfloat16, gdtype=F32)) == -4 and call(problem(gdtype=F64)) == -4    # INTERPOL_E_DTYPE
    assert call(problem(C=0)) == -5 and call(problem(B=0)) == -5 and call(problem(B=65536)) == -5       # INTERPOL_E_SHAPE
    assert call(problem(C=2)) == -5                                     # one channel
    for nb in (7, 65, 0, -1):
        assert call(problem(), nb=nb) == -5                             # 8 <= bins <= 64
    for kind in (-1, 3):
        assert call(problem(), kind=kind) == -5                         # hessian_kind
    assert call(problem(extrapolate=3)) == -7                           # INTERPOL_E_EXTRAP
    assert call(problem(fstr=[fixed.stride(0), 1, 4, 28, 7, 0, 0])) == -10    # a fixed image that is not row-major: INTERPOL_E_STRIDE
    assert call(problem(dstr=[disp.stride(0), 28, 7, 1, N])) == -10     # a channel-first displacement
    assert call(problem(flags=_hip.FLAG_SEPARABLE_GRID)) == -10 and call(problem(flags=_hip.FLAG_AFFINE_GRID)) == -10
    assert call(problem(), wbs=-1) == -10 and call(problem(), gbs=3 * N - 1) == -10 and call(problem(), hbs=-1) == -10
    assert call(problem(), g=disp) == -10                               # the gradient is the displacement
    assert call(problem(), g=moving.view(-1)[7:]) == -10                # ... starts inside the moving image
    assert call(problem(), h=fixed) == -10 and call(problem(), lo=weight) == -10
    assert call(problem(), hi=moving) == -10 and call(problem(), lo=ranges.view(torch.float32)) == -10   # the histogram, the ranges
    assert call(problem(), h=grad.view(-1), hbs=3 * N, kind=1) == -10   # two outputs that are one buffer
    assert call(problem(), lo=hess.view(-1)[11:]) == -10 and call(problem(), hi=hess.view(-1)) == -10
    assert call(problem(), work=hess.view(torch.uint8), nbytes=need) == -10           # the workspace is an output
    assert call(problem(), work=moving.view(torch.uint8), nbytes=need) == -10         # ... an input
    big = torch.zeros(need + 8, dtype=torch.uint8, device=DEV)
    assert call(problem(), work=big[4:], nbytes=need) == -10            # a workspace that is not 8-byte aligned
    assert call(problem(), nbytes=need - 1) == -9                       # INTERPOL_E_SCRATCH
    for missing in ("m", "f", "u", "r", "lo", "g", "h"):
        assert call(problem(), **{missing: None}) == -6                 # INTERPOL_E_NULL
    assert call(problem(), work=None, nbytes=need) == -6
    assert L.interpol_mi(None, *[ctypes.c_void_p(0)] * 9, 2, bins, 0, 0, 0, ctypes.c_void_p(0), 0, ctypes.c_void_p(0)) == -6
    torch.cuda.synchronize()
    assert all(bool((t == sentinel).all()) for t in (loss, grad, hess, hist)) and not bool(ws.any())
    # valid calls: as the binding makes them; a NULL weight, a NULL histogram and a NULL Hessian with no Hessian asked for
    ref = _hip.mi(moving, fixed, disp, weight, ranges, [3] * 3, [3] * 3, 1, "full", bins, True)
    assert call(problem()) == 0
    torch.cuda.synchronize()
    assert torch.equal(loss, ref[0]) and torch.equal(grad, ref[1]) and torch.equal(hess, ref[2]) and torch.equal(hist, ref[3]) and bool(ws.any())
    hess.fill_(sentinel)
    hist.fill_(sentinel)
    r1 = torch_kernels.mi_ranges(moving, fixed, None, None, (0, bins - 1), 2)
    assert call(problem(), w=None, r=r1, h=None, hi=None, kind=0, wbs=-1, hbs=-1) == 0
    torch.cuda.synchronize()
    assert torch.equal(grad, _hip.mi(moving, fixed, disp, None, r1, [3] * 3, [3] * 3, 1, None, bins, False)[1])
    assert bool((hess == sentinel).all()) and bool((hist == sentinel).all())


# ---------------------------------------------------------------------------------------------------------------------
# 6. descent on the device
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_descent(dtype, monkeypatch):
    route_all(monkeypatch)
    calls = fused_calls(monkeypatch)
    moving, fixed, _ = aff.field(dtype, DEV)
    totals = cpu.descend(moving, fixed)
    print("descent on the device %s: loss + energy from %.6g to %.6g (the composed form in float64 on the CPU: %.6g to %.6g)"
          % (dtype, totals[0], totals[-1], *cpu.DESCENT_MEASURED))
    assert calls["n"] == cpu.DESCENT_ITERATIONS + 1
    assert totals[-1] - totals[0] <= cpu.descent_bar()
