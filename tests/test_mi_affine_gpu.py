"""`interpol.mi_gauss_newton_affine` on the device (csrc/mi_affine.hip).

Truth: the composed form in float64 on the CPU, fed the upcast inputs (tests/test_mi_affine_cpu.py: `truth_and_allowance`).  The
matrices have dyadic entries (multiples of 1/32), so every coordinate is exact in float32: both sides see the same `floor` and
the same mask.  The fixed images hold k + delta with integer k and dyadic |delta| <= 1/4 under an explicit fixed_range = (0, B - 1):
no sample sits near a bin edge, the float32 and the float64 side pick the same bin (asserted on the CPU: no sample is excluded).

Allowance per entry (derived in `truth_and_allowance`): tol = 1e-5 (float32) / 1e-11 (float64) times A = 1 + (B - 4) max|moving| /
(m_hi - m_lo), the amplification of an error in I into u; P: tol A P + N q / (2 W); loss, gradient and Hessian: the project's
per-sample bar summed over the samples with tol A in the place of tol.  The bar for P is relative to the bin, and the weight of a
tap at the end of the cubic B-spline's support is ill-conditioned in u: the kernels form the histogram in double (csrc/mi_affine.hip).

Lattices (moving -> fixed), each for a way the reduction can go wrong: 1x1x1 and 2x1x1 leave all but one workgroup without a sample;
5x6x7 is a single partial workgroup; 9x33x70 is not a multiple of 256 and leaves most workgroups empty; 40x96x72 has 276 480
samples, more than 1024 * 256, so every workgroup loops; 33x70 and 600x450, 7 and 300 000 are their 2-D and 1-D counterparts.
"""
import ctypes

import pytest
import torch

import interpol
from interpol import _hip, backend, ops, torch_kernels
import memguard
import test_mi_affine_cpu as cpu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = {torch.float32: 1e-5, torch.float64: 1e-11}
F32, F64 = torch.float32, torch.float64
ALL_ORDERS = (1, 2, 3)

# (moving, fixed lattice, dtype, order, bound, extrapolate, bins, weighted, hessian, moving_range)
PARITY = [
    ((3, 2, 2), (1, 1, 1), F64, 1, "dct2", True, 8, False, True, None),
    ((3, 2, 2), (2, 1, 1), F32, 2, "dft", False, 32, True, True, None),
    ((7, 5, 6), (5, 6, 7), F64, 3, "zero", False, 8, True, True, None),
    ((7, 5, 6), (5, 6, 7), F32, 1, "replicate", 2, 64, False, False, (-1.0, 1.5)),
    ((12, 30, 64), (9, 33, 70), F64, 2, "replicate", 2, 32, True, True, (-1.0, 1.5)),
    ((44, 90, 80), (40, 96, 72), F32, 3, "dct2", True, 32, True, True, None),
    ((44, 90, 80), (40, 96, 72), F64, 1, "dft", False, 64, False, True, None),
    ((40, 64), (33, 70), F64, 3, "dft", False, 8, True, False, None),
    ((40, 64), (33, 70), F32, 2, "zero", True, 32, False, True, None),
    ((512, 512), (600, 450), F32, 1, "dct2", False, 64, True, True, None),
    ((512, 512), (600, 450), F64, 2, "zero", 2, 32, False, True, (-2.0, 2.0)),
    ((9,), (7,), F64, 3, "replicate", True, 8, True, True, None),
    ((270000,), (300000,), F32, 2, "dct2", True, 64, False, True, None),
    ((250000,), (300000,), F64, 1, "zero", False, 32, True, True, None),
]


def case_id(c):
    return "%s-%s-o%d-%s-e%d-B%d%s%s%s" % ("x".join(map(str, c[1])), "f32" if c[2] == F32 else "f64", c[3], c[4], int(c[5]), c[6],
                                           "-w" if c[7] else "", "" if c[8] else "-nohess", "-range" if c[9] else "")


def fused_calls(monkeypatch):
    """count the calls that reach the binding of the library"""
    calls = dict(n=0)
    fn = _hip.mi_affine

    def f(*a, **k):
        calls["n"] += 1
        return fn(*a, **k)

    monkeypatch.setattr(_hip, "mi_affine", f)
    return calls


def route_all(monkeypatch):
    monkeypatch.setattr(backend, "fused_mi_affine_orders", ALL_ORDERS)


def dev(t):
    return None if t is None else t.to(DEV)


def same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


def no_sample_near_a_bin_edge(fixed, bins):
    t = fixed.double() / (bins - 1) * (bins - 1)
    return bool(((t - t.round()).abs() <= 0.25 + 1e-9).all()) and bool((fixed >= 0).all()) and bool((fixed <= bins - 1).all())


def check(got, want, allow, what, hessian=True):
    ratios = dict(loss=cpu.worst_ratio(got[0], want[0], allow[0]), gradient=cpu.worst_ratio(got[1], want[1], allow[1]),
                  P=cpu.worst_ratio(got[3], want[3], allow[3]))
    if hessian:
        ratios["hessian"] = cpu.worst_ratio(got[2], want[2], allow[2])
        assert torch.equal(got[2], got[2].mT), what
    else:
        assert got[2] is None, what
    print("parity %s: worst error / allowance: %s" % (what, ", ".join("%s %.3g" % kv for kv in ratios.items())))
    assert all(v <= 1.0 for v in ratios.values()), (what, ratios)
    return ratios


# ---------------------------------------------------------------------------------------------------------------------
# 1. parity with the composed form in float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PARITY, ids=case_id)
def test_parity_with_the_composed_form_in_float64(case, monkeypatch):
    inshape, shape, dtype, order, bound, extrapolate, bins, weighted, hessian, mrange = case
    route_all(monkeypatch)
    calls = fused_calls(monkeypatch)
    dim = len(shape)
    moving, fixed, weight = cpu.problem(inshape, shape, 1000 + PARITY.index(case), dtype, bins=bins, B=1, weighted=weighted)
    assert no_sample_near_a_bin_edge(fixed, bins)
    mat = cpu.matrix(dim, dtype)[None]
    kw = dict(interpolation=order, bound=bound, extrapolate=extrapolate)
    mi = dict(bins=bins, moving_range=mrange, fixed_range=(0, bins - 1))
    want, allow = cpu.truth_and_allowance(moving, fixed, mat, weight, TOL[dtype], **mi, **kw)
    if extrapolate is False and max(shape) > 2:                           # part of the lattice is out of view, part of it in view
        from interpol.sepgrid import AffineGrid
        x = AffineGrid(mat[0].double(), shape).dense()[0]
        inside = ((x > -0.05) & (x < torch.tensor(inshape) - 0.95)).all(-1).double().mean()
        assert 0.0 < float(inside) < 1.0, float(inside)
    got = interpol.mi_gauss_newton_affine(dev(moving), dev(fixed), dev(mat), dev(weight), hessian=hessian, return_histogram=True, **mi, **kw)
    assert calls["n"] == 1
    P = dim * (dim + 1)
    assert got[0].shape == (1,) and got[1].shape == (1, dim, dim + 1) and (not hessian or got[2].shape == (1, P, P))
    assert got[3].shape == (1, bins, bins)
    assert all(t.dtype == dtype and t.is_cuda for t in got if t is not None)
    check(got, want, allow, case_id(case), hessian)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_three_matrices_a_shared_moving_image_and_a_batched_weight(dtype, monkeypatch):
    """The first combination (float32: shared moving image, three matrices, batched weight) has a nearly empty bin, P = 1.7e-9,
    filled by samples whose u lies a few 1e-4 past a knot: their weight e^3 / 6 has the relative sensitivity 3 / e to u.  With I and u
    in float32 that bin came to 1.71 of its bar (as the composed form in float32 does on the CPU); the histogram stage evaluates
    them in double from the tensors' values and stays at 0.002."""
    route_all(monkeypatch)
    calls = fused_calls(monkeypatch)
    bins = 8
    moving, fixed, weight = cpu.problem((7, 5, 6), (5, 6, 7), 1100, dtype, bins=bins, B=3)
    mats = torch.stack([cpu.matrix(3, dtype, s) for s in (1.0, 0.5, -0.25)])
    mats[1, 0, 0] += 0.0625
    kw = dict(interpolation=2, bound="dct2", extrapolate=False)
    mi = dict(bins=bins, moving_range=None, fixed_range=(0, bins - 1))
    for m, f, a, w in ((moving[:1], fixed, mats, weight), (moving[:1], fixed[:1], mats[:1], weight), (moving, fixed[:1], mats, None)):
        want, allow = cpu.truth_and_allowance(m, f, a, w, TOL[dtype], **mi, **kw)
        got = interpol.mi_gauss_newton_affine(dev(m), dev(f), dev(a), dev(w), return_histogram=True, **mi, **kw)
        assert got[0].shape == (3,) and got[2].shape == (3, 12, 12) and got[3].shape == (3, bins, bins)
        check(got, want, allow, "B=3 %s moving %d fixed %d mat %d weight %s" % (dtype, m.shape[0], f.shape[0], a.shape[0], w is not None))
    assert calls["n"] == 3


# ---------------------------------------------------------------------------------------------------------------------
# 2. routing
# ---------------------------------------------------------------------------------------------------------------------
def test_default_routing_reaches_the_fused_kernels_once(monkeypatch):
    calls = fused_calls(monkeypatch)
    assert isinstance(backend.fused_mi_affine_orders, tuple) and set(backend.fused_mi_affine_orders) <= set(ALL_ORDERS)
    for (inshape, shape), dtype in ((((7, 5, 6), (5, 6, 7)), F32), (((40, 64), (33, 70)), F64), (((9,), (7,)), F32)):
        dim = len(shape)
        moving, fixed, weight = (dev(t) for t in cpu.problem(inshape, shape, 1200, dtype, B=2))
        mat = dev(cpu.matrix(dim, dtype))
        for order in ALL_ORDERS:
            routed = order in backend.fused_mi_affine_orders
            assert ops.mi_affine_covered(moving, fixed, mat[None], weight, [order], 32) == routed
            before = calls["n"]
            loss, g, h = interpol.mi_gauss_newton_affine(moving, fixed, mat, weight, interpolation=order)
            assert calls["n"] - before == routed
            assert loss.shape == (2,) and g.shape == (2, dim, dim + 1) and h.shape == (2, dim * (dim + 1), dim * (dim + 1))
            assert all(t.dtype == dtype and t.is_cuda for t in (loss, g, h))


@pytest.mark.parametrize("what", ["bf16", "4d", "mixed_orders", "many_bins", "switched_off"])
def test_uncovered_classes_take_the_composed_route(what, monkeypatch):
    """Each case differs from a call that reaches the fused kernels in ONE property; the control is asserted to reach the binding."""
    route_all(monkeypatch)
    calls = fused_calls(monkeypatch)
    control = [dev(t) for t in cpu.problem((7, 5, 6), (5, 6, 7), 1300, F32)]
    cmat = dev(cpu.matrix(3, F32, 0.25))
    interpol.mi_gauss_newton_affine(control[0], control[1], cmat, control[2], interpolation=1, bins=8)
    assert calls["n"] == 1
    order = [1, 2, 3] if what == "mixed_orders" else 1
    bins = 65 if what == "many_bins" else 8
    if what == "4d":
        gen = torch.Generator().manual_seed(5)
        moving, fixed, weight = torch.randn(2, 1, 4, 3, 4, 3, generator=gen), cpu.binned((3, 4, 3, 2), 8, gen, [2, 1]).float(), None
        mat = torch.eye(5)[:4] + 0.0625 * torch.randn(4, 5, generator=gen).round()
    else:
        moving, fixed, weight = cpu.problem((7, 5, 6), (5, 6, 7), 1300, torch.bfloat16 if what == "bf16" else F32)
        mat = cpu.matrix(3, moving.dtype, 0.25)
    if what == "switched_off":
        monkeypatch.setattr(backend, "fused_mi_affine_orders", ())
    kw = dict(interpolation=order, bound="dct2", extrapolate=True, bins=bins)
    got = interpol.mi_gauss_newton_affine(dev(moving), dev(fixed), dev(mat), dev(weight), **kw)
    assert calls["n"] == 1 and all(t.dtype == moving.dtype and t.is_cuda for t in got)
    want = interpol.mi_gauss_newton_affine(moving.double(), fixed.double(), mat.double(), None if weight is None else weight.double(), **kw)
    tol = 2e-2 if what == "bf16" else 1e-4                                 # relative to the largest entry: the composed route in float32
    for g, w in zip(got, want):
        assert float((g.double().cpu() - w).abs().max()) <= tol * float(w.abs().max()), what


# ---------------------------------------------------------------------------------------------------------------------
# 3. bits
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_bits_do_not_depend_on_the_run_or_on_the_batch(dtype, monkeypatch):
    route_all(monkeypatch)
    for inshape, shape, order, hessian, bins in (((7, 5, 6), (5, 6, 7), 3, True, 8), ((12, 30, 64), (9, 33, 70), 1, True, 32),
                                                 ((40, 64), (33, 70), 2, False, 64), ((9,), (300,), 2, True, 16)):
        dim = len(shape)
        moving, fixed, weight = (dev(t) for t in cpu.problem(inshape, shape, 1400, dtype, bins=bins, B=3))
        mats = dev(torch.stack([cpu.matrix(dim, dtype, s) for s in (1.0, 0.5, -0.25)]))
        kw = dict(interpolation=order, bound="dct2", extrapolate=False, hessian=hessian, bins=bins, return_histogram=True)
        a = interpol.mi_gauss_newton_affine(moving, fixed, mats, weight, **kw)
        b = interpol.mi_gauss_newton_affine(moving, fixed, mats, weight, **kw)
        assert same(a, b), (shape, order)
        assert bool((a[0] < 0).all()) and bool(a[1].isfinite().all())
        if hessian:
            assert torch.equal(a[2], a[2].mT) and bool(a[2].isfinite().all())
        for i in (0, 2):
            one = interpol.mi_gauss_newton_affine(moving[i], fixed[i], mats[i], weight[i], **kw)
            assert same(one, [None if t is None else t[i] for t in a]), (shape, order, i)


def test_graph_replay_gives_the_bits_of_eager(monkeypatch):
    route_all(monkeypatch)
    moving, fixed, weight = (dev(t) for t in cpu.problem((12, 30, 64), (9, 33, 70), 1500, F32, bins=32, B=2))
    mat = dev(torch.stack([cpu.matrix(3, F32), cpu.matrix(3, F32, 0.5)]))
    kw = dict(interpolation=3, bound="dct2", extrapolate=True, bins=32, return_histogram=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                        # warm-up on the side stream (module loads)
        interpol.mi_gauss_newton_affine(moving, fixed, mat, weight, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = interpol.mi_gauss_newton_affine(moving, fixed, mat, weight, **kw)
    for it in range(3):
        mat[:, :, -1] += 0.5 * (it + 1)
        graph.replay()
        torch.cuda.synchronize()
        eager = interpol.mi_gauss_newton_affine(moving, fixed, mat, weight, **kw)
        assert same(out, eager), it
        assert bool(out[0].isfinite().all()) and bool((out[0] < 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# 4. memory contract
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("misalign", [0, 1, 3])
def test_memory_contract(misalign, dtype):
    for inshape, shape, hessian, bins in (((7, 5, 6), (5, 6, 7), True, 8), ((12, 30, 64), (9, 33, 70), True, 64), ((40, 64), (33, 70), False, 32),
                                          ((9,), (7,), True, 9)):
        dim = len(shape)
        moving, fixed, weight = cpu.problem(inshape, shape, 1600, dtype, bins=bins, B=2)
        mat = torch.stack([cpu.matrix(dim, dtype), cpu.matrix(dim, dtype, 0.5)])
        args = [moving, fixed, mat, weight]
        ranges = torch_kernels.mi_ranges(dev(moving), dev(fixed), dev(weight), None, (0, bins - 1), 2)
        for bound, extrapolate in ((3, 1), (6, 0)):
            opt = ([bound] * 3, [3] * 3, extrapolate, hessian, bins, True)
            ref = _hip.mi_affine(*[dev(t) for t in args], ranges, *opt)
            assert all(bool(torch.isfinite(r).all()) for r in ref if r is not None)
            with memguard.installed(_hip, misalign=misalign) as seam:
                placed = [memguard.place(t, DEV, misalign=misalign) for t in args]
                out = _hip.mi_affine(*placed, ranges, *opt)
                torch.cuda.synchronize()
                what = (shape, bound, misalign)
                assert len(seam.outputs()) == 3 + hessian and len(seam.workspaces()) == 1 and seam.workspace_was_written(), what
                P = dim * (dim + 1)
                assert out[0].shape == (2,) and out[1].shape == (2, dim, dim + 1) and (not hessian or out[2].shape == (2, P, P)), what
                assert out[3].shape == (2, bins, bins), what
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
def raw_call(L, p, moving, fixed, mat, weight, ranges, loss, grad, hess, hist, with_hessian, bins, mbs, wbs, ws, nbytes=None):
    ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)
    return L.interpol_mi_affine(ctypes.byref(p), ptr(moving), ptr(fixed), ptr(mat), ptr(weight), ptr(ranges), ptr(loss), ptr(grad),
                                ptr(hess), ptr(hist), with_hessian, bins, mbs, wbs, ptr(ws),
                                (0 if ws is None else ws.numel()) if nbytes is None else nbytes, ctypes.c_void_p(0))


def test_entry_points_validate_before_launching():
    L = _hip.lib()
    inshape, shape, bins = (6, 5, 4), (5, 4, 7), 16
    N = 5 * 4 * 7
    moving, fixed, weight = (dev(t) for t in cpu.problem(inshape, shape, 1800, F32, bins=bins, B=2))
    mat = dev(torch.stack([cpu.matrix(3, F32), cpu.matrix(3, F32, 0.5)]))
    ranges = torch_kernels.mi_ranges(moving, fixed, weight, None, (0, bins - 1), 2)
    sentinel = 4321.0
    loss = torch.full([2], sentinel, device=DEV)
    grad = torch.full([2, 3, 4], sentinel, device=DEV)
    hess = torch.full([2, 12, 12], sentinel, device=DEV)
    hist = torch.full([2, bins, bins], sentinel, device=DEV)

    def problem(dtype=F32, gdtype=None, dim=3, order=(3, 3, 3), bound=3, extrapolate=1, C=1, B=2, mstr=None, fstr=None,
                flags=_hip.FLAG_AFFINE_GRID, inshp=inshape, shp=shape):
        m = mstr or [moving.stride(0), moving.stride(1), *moving.stride()[2:]]
        f = fstr or [fixed.stride(0), fixed.stride(1), *fixed.stride()[2:], 0, 0]
        return _hip.make_problem(dim, dtype, gdtype or dtype, [bound] * 3, list(order), extrapolate, B, C, inshp, shp, m, [0] * 5, f, flags)

    need = L.interpol_mi_affine_workspace(ctypes.byref(problem()), bins)
    assert need == 2 * (2 * bins * bins * 8 + 8 + 73 * 1024 * 8)         # two tables, 1 / W and 73 sums of 1024 workgroups per item
    assert L.interpol_mi_affine_workspace(ctypes.byref(problem(dim=2, fstr=[0, 0, 4, 1, 0, 0, 0])), 64) == 2 * (2 * 64 * 64 * 8 + 8 + 25 * 1024 * 8)
    assert L.interpol_mi_affine_workspace(ctypes.byref(problem(dim=1, fstr=[0, 0, 1, 0, 0, 0, 0])), 8) == 2 * (2 * 8 * 8 * 8 + 8 + 6 * 1024 * 8)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)

    def call(p, m=moving, f=fixed, a=mat, w=weight, r=ranges, lo=loss, g=grad, h=hess, hi=hist, wh=1, nb=bins, mbs=12, wbs=N, work=ws,
             nbytes=None):
        return raw_call(L, p, m, f, a, w, r, lo, g, h, hi, wh, nb, mbs, wbs, work, nbytes)

    for dim in (0, 4):
        assert call(problem(dim=dim)) == -1 and L.interpol_mi_affine_workspace(ctypes.byref(problem(dim=dim)), bins) == -1   # INTERPOL_E_DIM
    for order in ((0, 0, 0), (4, 4, 4), (1, 2, 3), (3, 3, 1), (8, 8, 8), (-1, -1, -1)):
        assert call(problem(order=order)) == -2                         # INTERPOL_E_ORDER: one order 1..3
        assert L.interpol_mi_affine_workspace(ctypes.byref(problem(order=order)), bins) == -2
    for bound in (-1, 7):
        assert call(problem(bound=bound)) == -3                         # INTERPOL_E_BOUND
    for dtype in (torch.bfloat16, torch.float16):
        assert call(problem(dtype=dtype, gdtype=F32)) == -4             # INTERPOL_E_DTYPE
    assert call(problem(gdtype=F64)) == -4 and call(problem(dtype=F64, gdtype=F32)) == -4
    assert call(problem(C=0)) == -5 and call(problem(B=0)) == -5 and call(problem(B=65536)) == -5   # INTERPOL_E_SHAPE
    assert call(problem(C=2)) == -5 and L.interpol_mi_affine_workspace(ctypes.byref(problem(C=2)), bins) == -5   # one channel
    for nb in (7, 65, 0, -1):
        assert call(problem(), nb=nb) == -5 and L.interpol_mi_affine_workspace(ctypes.byref(problem()), nb) == -5   # 8 <= bins <= 64
    assert call(problem(inshp=(6, 0, 4))) == -5
    assert call(problem(shp=(1 << 16, 1 << 16, 2), fstr=[0, 0, 1 << 17, 2, 1, 0, 0])) == -5               # 2^33 samples
    for wh in (-1, 2):
        assert call(problem(), wh=wh) == -5                             # with_hessian
    for extrapolate in (-1, 3):
        assert call(problem(extrapolate=extrapolate)) == -7             # INTERPOL_E_EXTRAP
    assert call(problem(fstr=[fixed.stride(0), 1, 4, 28, 7, 0, 0])) == -10    # a fixed image that is not row-major: INTERPOL_E_STRIDE
    assert call(problem(mstr=[moving.stride(0), moving.stride(1), -20, 4, 1])) == -10
    assert call(problem(mstr=[-1, moving.stride(1), 20, 4, 1])) == -10
    assert call(problem(fstr=[-1, fixed.stride(1), 28, 7, 1, 0, 0])) == -10
    assert call(problem(flags=_hip.FLAG_SEPARABLE_GRID)) == -10 and call(problem(flags=_hip.FLAG_DISPLACEMENT)) == -10
    assert call(problem(), mbs=-1) == -10 and call(problem(), wbs=-1) == -10
    assert call(problem(), g=mat) == -10                                # the gradient is the matrix
    assert call(problem(), g=moving.view(-1)[7:]) == -10                # ... starts inside the moving image
    assert call(problem(), h=fixed) == -10 and call(problem(), lo=weight) == -10
    assert call(problem(), hi=moving) == -10 and call(problem(), lo=ranges.view(torch.float32)) == -10   # the histogram, the ranges
    assert call(problem(), h=grad.view(-1)) == -10                      # two outputs that overlap
    assert call(problem(), lo=hess.view(-1)[11:]) == -10 and call(problem(), hi=hess.view(-1)) == -10
    assert call(problem(), work=hess.view(torch.uint8), nbytes=need) == -10           # the workspace is an output
    assert call(problem(), work=moving.view(torch.uint8), nbytes=need) == -10         # ... an input
    big = torch.zeros(need + 8, dtype=torch.uint8, device=DEV)
    assert call(problem(), work=big[4:], nbytes=need) == -10            # a workspace that is not 8-byte aligned
    odd = torch.zeros(11, dtype=torch.float32, device=DEV)
    if odd.data_ptr() % 8 == 0:
        assert call(problem(), r=odd[1:]) == -10                        # ranges that are not 8-byte aligned
    assert call(problem(), nbytes=need - 1) == -9                       # INTERPOL_E_SCRATCH
    for missing in ("m", "f", "a", "r", "lo", "g", "h"):
        assert call(problem(), **{missing: None}) == -6                 # INTERPOL_E_NULL
    assert call(problem(), work=None, nbytes=need) == -6
    assert L.interpol_mi_affine(None, *[ctypes.c_void_p(0)] * 9, 1, bins, 0, 0, ctypes.c_void_p(0), 0, ctypes.c_void_p(0)) == -6
    torch.cuda.synchronize()
    assert all(bool((t == sentinel).all()) for t in (loss, grad, hess, hist)) and not bool(ws.any())
    # valid calls: as the binding makes them; a NULL weight, a NULL histogram and a NULL Hessian with no Hessian asked for
    ref = _hip.mi_affine(moving, fixed, mat, weight, ranges, [3] * 3, [3] * 3, 1, True, bins, True)
    assert call(problem()) == 0
    torch.cuda.synchronize()
    assert torch.equal(loss, ref[0]) and torch.equal(grad, ref[1]) and torch.equal(hess, ref[2]) and torch.equal(hist, ref[3]) and bool(ws.any())
    hess.fill_(sentinel)
    hist.fill_(sentinel)
    r1 = torch_kernels.mi_ranges(moving, fixed, None, None, (0, bins - 1), 2)
    assert call(problem(), w=None, r=r1, h=None, hi=None, wh=0, wbs=-1) == 0
    torch.cuda.synchronize()
    assert torch.equal(grad, _hip.mi_affine(moving, fixed, mat, None, r1, [3] * 3, [3] * 3, 1, False, bins, False)[1])
    assert bool((hess == sentinel).all()) and bool((hist == sentinel).all())


# ---------------------------------------------------------------------------------------------------------------------
# 6. recovery of a known matrix on the device
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_recovery_of_a_known_matrix(dtype, monkeypatch):
    route_all(monkeypatch)
    calls = fused_calls(monkeypatch)
    errors = cpu.recover(*cpu.field(dtype, DEV))
    print("recovery on the device %s: max matrix error at the start %.3g, after %d iterations %.3g (ratio %.3g)"
          % (dtype, errors[0], cpu.RECOVERY_ITERATIONS, errors[-1], errors[-1] / errors[0]))
    assert calls["n"] == cpu.RECOVERY_ITERATIONS
    assert errors[-1] / errors[0] <= cpu.recovery_bar()
