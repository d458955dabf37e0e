"""`interpol.lcc_gauss_newton` on the device (csrc/lcc.hip).

Truth: the definition restated in tests/test_lcc_cpu.py (`truth`), evaluated on the CPU in float64 on the inputs as the device sees
them (rounded to its dtype) and at the coordinates o + disp formed in the device's precision, then widened; never the code under
test.  Coordinates within 1e-3 of a spline knot or of a half-integer are moved by 2^-7 before either side sees them (`nudged`).
Nothing is masked out of the comparison.

Bar: |got - want| <= tol |want| + tol scale, tol = 1e-5 (float32) / 1e-11 (float64); scale = max |want| of that output over the
batch item, 0 for the loss.

Compared groups: (offset 0, eps 1e-5), (offset 0, eps 1), (offset 10, eps 1).  The group (offset 10, eps 1e-5) is NOT compared:
there den falls to eps in low-contrast windows, where the float32 rounding of I alone -- before any arithmetic of the kernel --
moves cross^2 / den by more than the bar (an emulation of the precision contract on the CPU reaches 34 times the bar).

The window-sum tile of csrc/lcc.hip is 8 x 32 columns (y, z) marched over chunks of 32 planes along x; a lattice with fewer dims
has leading extents of 1.  (33, 9, 33) is one past the tile and the chunk on every axis, (9, 33) and (257,) likewise in 2-D and 1-D.
Shapes (moving -> fixed): (300,) -> (257,), (9, 12) -> (8, 13), (5, 3, 33) -> (5, 3, 33), (10, 9, 40) -> (9, 10, 36), (1, 2, 3) ->
(2, 1, 3) (every extent is 1, or a window swallows the axis: 9 on an extent of 2) and (30, 8, 35) -> (33, 9, 33).  Windows: 3, 5, 9,
the mixed [3, 9, 5] and one with a 1 in a dimension.  Under extrapolate = False sigma = 0.4, and at least 40 % of the samples of
the four larger shapes are in view.

Measured on an MI355X, worst error / bar over all cases (loss, gradient, hessian) -- float32: (0, 1e-5) 0.017, 0.45, 0.64; (0, 1)
0.008, 0.021, 0.025; (10, 1) 0.78, 0.21, 0.40.  float64: (0, 1e-5) 5e-4, 0.005, 0.004; (0, 1) 2e-4, 1e-4, 1e-4; (10, 1) 0.45, 0.11, 0.26.
(With the second moments of the truth in their plain form, and plain double sums in the kernel, the float64 gradient of (300,) ->
(257,), order 2, window 3, eps 1e-5 stood at 1.47 of the bar: 0.46 of it the truth's own cancellation, measured against a long-double
evaluation.  The truth now sums them in their central form for small windows, the kernel carries the rounding errors of its sums.)
"""
import ctypes
import itertools

import pytest
import torch

import interpol
from interpol import _hip, backend, ops
import memguard
import test_ssd_cpu as ssd
import test_lcc_cpu as cpu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = {torch.float32: 1e-5, torch.float64: 1e-11}
SHAPES = [((300,), (257,)), ((9, 12), (8, 13)), ((5, 3, 33), (5, 3, 33)), ((10, 9, 40), (9, 10, 36)), ((1, 2, 3), (2, 1, 3)),
          ((30, 8, 35), (33, 9, 33))]
TINY = [((1, 2, 3), (2, 1, 3))]
IDS = ssd.IDS(SHAPES)
ALL_ORDERS = (1, 2, 3)
GROUPS = ((0.0, 1e-5), (0.0, 1.0), (10.0, 1.0))                         # (offset, eps)
WINDOWS = (3, 5, 9, [3, 9, 5], [5, 1, 3])


def fused_calls(monkeypatch):
    """count the calls that reach the binding of the library"""
    calls = dict(lcc=0)
    fn = _hip.lcc

    def f(*a, **k):
        calls["lcc"] += 1
        return fn(*a, **k)

    monkeypatch.setattr(_hip, "lcc", f)
    return calls


def route_all(monkeypatch):
    monkeypatch.setattr(backend, "fused_lcc_orders", ALL_ORDERS)


def dev(t):
    return None if t is None else t.to(DEV)


def on_device(args):
    return [dev(t) for t in args]


def folded(args):
    return [args[0], args[1][None], args[2], args[3]]


def window_of(window, dim):
    """the first `dim` entries of a per-dimension list (the LAST of the one with a 1, so that two dimensions keep it)"""
    if not isinstance(window, list):
        return window
    return window[-dim:] if 1 in window else window[:dim]


def same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------------
# 1. routing
# ---------------------------------------------------------------------------------------------------------------------
def test_default_routing_reaches_the_fused_kernel_once(monkeypatch):
    calls = fused_calls(monkeypatch)
    assert isinstance(backend.fused_lcc_orders, tuple) and set(backend.fused_lcc_orders) <= set(ALL_ORDERS)
    for (inshape, shape), dtype in itertools.product(SHAPES[:3], (torch.float32, torch.float64)):
        args = on_device(cpu.problem(inshape, shape, 1, dtype))
        for order in backend.fused_lcc_orders:
            assert ops.lcc_covered(*folded(args), [order], [5])
            before = calls["lcc"]
            loss, g, h = interpol.lcc_gauss_newton(*args, window=5, interpolation=order)
            assert calls["lcc"] - before == 1
            assert loss.shape == (2,) and g.shape == args[2].shape and h.shape[:-1] == g.shape[:-1]
            assert all(t.dtype == dtype and t.is_cuda for t in (loss, g, h))
    for order in ALL_ORDERS:
        before = calls["lcc"]
        interpol.lcc_gauss_newton(*args, interpolation=order, hessian=None)
        assert calls["lcc"] - before == (order in backend.fused_lcc_orders)


@pytest.mark.parametrize("what", ["bf16", "4d", "mixed_orders", "window_11", "switched_off"])
def test_uncovered_classes_take_the_composed_route(what, monkeypatch):
    """Each case differs from a call that reaches the fused kernels in ONE property; the control -- the same call without the
    property -- is asserted to reach the binding."""
    monkeypatch.setattr(backend, "fused_lcc_orders", (1,))
    inshape, shape = ((3, 2, 4, 3), (2, 3, 3, 2)) if what == "4d" else ((10, 9, 14), (9, 10, 12))
    dtype = torch.bfloat16 if what == "bf16" else torch.float32
    args = cpu.problem(inshape, shape, 3, dtype, sigma=0.7)
    order = [1, 2, 3] if what == "mixed_orders" else 1
    window = 11 if what == "window_11" else 3
    kw = dict(interpolation=order, bound="dct2", extrapolate=True, window=window, eps=1e-2)
    calls = fused_calls(monkeypatch)
    control = cpu.problem((10, 9, 14), (9, 10, 12), 3, torch.float32, sigma=0.7) if what == "4d" else [t.float() for t in args]
    assert ops.lcc_covered(*folded(on_device(control)), [1], [3])
    interpol.lcc_gauss_newton(*on_device(control), **dict(kw, interpolation=1, window=3))
    assert calls["lcc"] == 1
    if what == "switched_off":
        monkeypatch.setattr(backend, "fused_lcc_orders", ())
    assert not ops.lcc_covered(*folded(on_device(args)), order if isinstance(order, list) else [order], [window])
    got = interpol.lcc_gauss_newton(*on_device(args), **kw)
    assert calls["lcc"] == 1 and all(t.dtype == dtype and t.is_cuda for t in got)
    want = cpu.truth(*[t.float() for t in args], **kw)                   # (the coordinates are formed in float32 on the device)
    tol = 1e-2 if what == "bf16" else TOL[torch.float32]
    # (16-bit: one rounding of each output on top of the float32 error)
    assert cpu.item_ratio(got[0], want[0], tol, False) <= 1.0
    assert cpu.item_ratio(got[1], want[1], tol) <= 1.0 and cpu.item_ratio(got[2], want[2], tol) <= 1.0


def test_extrapolate_0_1_2_is_the_mask_of_pull_and_grad():
    """the binding at every extrapolate against the definition on interpol_pull / interpol_grad with the same flag"""
    seen = {0: 0, 1: 0, 2: 0}
    for inshape, shape, order in (((10, 9, 14), (9, 10, 12), 3), ((9, 12), (8, 13), 2), ((11,), (9,), 1)):
        dim = len(shape)
        moving, fixed, disp, weight = cpu.problem(inshape, shape, 5, torch.float32, sigma=2.0)
        disp, _ = ssd.nudged(disp, order)
        moving, fixed, disp, weight = on_device((moving, fixed[None], disp, weight))
        window = [3] * dim
        for extrapolate in (0, 1, 2):
            opt = ([3] * dim, [order] * dim, extrapolate)
            loss, g, h = _hip.lcc(moving, fixed, disp, weight, *opt, "full", window, 1e-2)
            I = _hip.gather("pull", moving, disp, *opt, flags=_hip.FLAG_DISPLACEMENT).double().cpu()
            G = _hip.gather("grad", moving, disp, *opt, flags=_hip.FLAG_DISPLACEMENT).double().cpu()
            J, wt = fixed.double().cpu(), weight.double().cpu().unsqueeze(1)
            wcc, cross, vJ, den, n, SI, SJ, _ = cpu.cc_terms(I, J, weight.double().cpu(), window, 1e-2)
            a, c = wt * 2 * cross / den, wt * 2 * cross * cross * vJ / (den * den)
            f = (a * SJ - c * SI) / n
            A, C, F = (cpu.box(t, window) for t in (a, c, f))
            dI = -J * A + I * C + F
            pairs = [(d, d) for d in range(dim)] + [(d, e) for d in range(dim) for e in range(d + 1, dim)]
            assert cpu.item_ratio(loss, -wcc.flatten(1).sum(1), 1e-5, False) <= 1.0
            assert cpu.item_ratio(g, (dI.unsqueeze(-1) * G).sum(1), 1e-5) <= 1.0
            assert cpu.item_ratio(h, torch.stack([(C * G[..., d] * G[..., e]).sum(1) for d, e in pairs], -1), 1e-5) <= 1.0
            seen[extrapolate] += int((G != 0).any(-1).any(1).sum())
    assert seen[1] > seen[2] > seen[0] > 0, seen


# ---------------------------------------------------------------------------------------------------------------------
# 2. parity with the definition in float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", range(len(SHAPES)), ids=IDS)
def test_parity_with_the_definition_in_float64(case, dtype, monkeypatch):
    inshape, shape = SHAPES[case]
    dim = len(shape)
    route_all(monkeypatch)
    calls = fused_calls(monkeypatch)
    tol = TOL[dtype]
    worst = {g: dict(loss=0.0, gradient=0.0, hessian=0.0) for g in GROUPS}
    ccs, n_calls = [], 0
    for n, (order, window, group) in enumerate(itertools.product(ALL_ORDERS, WINDOWS, GROUPS)):
        offset, eps = group
        bound = ssd.BOUNDS[n % 7]
        extrapolate = (n // 3) % 2 == 0
        sigma = 0.4 if not extrapolate else (2.0, 0.4)[(n // 6) % 2]
        C, weighted = (1, 3)[n % 2], (n // 2) % 2 == 1
        window = window_of(window, dim)
        moving, fixed, disp, weight = cpu.problem(inshape, shape, 1000 * case + n, dtype, C=C, sigma=sigma, weighted=weighted,
                                                  offset=offset)
        disp, _ = ssd.nudged(disp, order)
        if not extrapolate and (inshape, shape) not in TINY:
            assert ssd.in_view(disp, inshape) >= 0.40, (inshape, shape, n)
        kw = dict(interpolation=order, bound=bound, extrapolate=extrapolate, window=window, eps=eps)
        want = cpu.truth(moving, fixed, disp, weight, hessian="full", **kw)
        ccs.append(want[3])
        kinds = ("full", "diagonal", None) if n == 4 * dim else ("full",)
        for kind in kinds:
            got = interpol.lcc_gauss_newton(dev(moving), dev(fixed), dev(disp), dev(weight), hessian=kind, **kw)
            n_calls += 1
            assert got[0].shape == (2,) and got[1].shape == disp.shape and all(t.dtype == dtype for t in got if t is not None)
            ratios = dict(loss=cpu.item_ratio(got[0], want[0], tol, False), gradient=cpu.item_ratio(got[1], want[1], tol))
            if kind is None:
                assert got[2] is None
            else:
                K = dim if kind == "diagonal" else want[2].shape[-1]
                assert got[2].shape == (2, *shape, K)
                ratios["hessian"] = cpu.item_ratio(got[2], want[2][..., :K], tol)
            for k, v in ratios.items():
                worst[group][k] = max(worst[group][k], v)
            print("parity %s->%s %s order %d %s extrapolate %d window %s offset %g eps %g C %d weight %d sigma %.1f %s: error / bar %s"
                  % (inshape, shape, dtype, order, bound, extrapolate, window, offset, eps, C, weighted, sigma, kind,
                     ", ".join("%s %.3g" % kv for kv in ratios.items())))
            assert all(v <= 1.0 for v in ratios.values()), (inshape, shape, dtype, kw, C, weighted, sigma, kind, ratios)
    for group in GROUPS:
        print("parity %s->%s %s offset %g eps %g: worst error / bar: loss %.3g, gradient %.3g, hessian %.3g"
              % (inshape, shape, dtype, *group, worst[group]["loss"], worst[group]["gradient"], worst[group]["hessian"]))
    print("mean cc between %.3g and %.3g" % (min(ccs), max(ccs)))
    assert calls["lcc"] == n_calls and max(ccs) > 1e-3                 # not zeros against zeros


# ---------------------------------------------------------------------------------------------------------------------
# 3. bits
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_bits_do_not_depend_on_the_run_or_on_the_batch(dtype, monkeypatch):
    route_all(monkeypatch)
    for ((inshape, shape), order, kind, window) in ((SHAPES[5], 3, "full", 9), (SHAPES[0], 2, "diagonal", 5), (SHAPES[1], 1, None, [3, 9]),
                                                    (SHAPES[3], 1, "full", [3, 9, 5])):
        moving, fixed, disp, weight = on_device(cpu.problem(inshape, shape, 40, dtype, B=3))
        fixed = fixed[None].expand(3, *fixed.shape).contiguous()
        kw = dict(interpolation=order, bound="dct2", extrapolate=False, hessian=kind, window=window)
        a = interpol.lcc_gauss_newton(moving, fixed, disp, weight, **kw)
        b = interpol.lcc_gauss_newton(moving, fixed, disp, weight, **kw)
        assert same(a, b), (shape, order)
        one = interpol.lcc_gauss_newton(moving[1:2], fixed[1:2], disp[1:2], weight[1:2], **kw)
        assert same([None if t is None else t[0] for t in one], [None if t is None else t[1] for t in a]), (shape, order)


def test_graph_replay_gives_the_bits_of_eager(monkeypatch):
    route_all(monkeypatch)
    inshape, shape = SHAPES[3]
    moving, fixed, disp, weight = on_device(cpu.problem(inshape, shape, 50, torch.float32))
    kw = dict(interpolation=3, bound="dct2", extrapolate=True, window=5)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                        # warm-up on the side stream (module loads)
        interpol.lcc_gauss_newton(moving, fixed, disp, weight, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = interpol.lcc_gauss_newton(moving, fixed, disp, weight, **kw)
    gen = torch.Generator().manual_seed(51)
    for it in range(3):
        disp.copy_(torch.randn(disp.shape, generator=gen) * (1 + it))
        graph.replay()
        torch.cuda.synchronize()
        eager = interpol.lcc_gauss_newton(moving, fixed, disp, weight, **kw)
        assert same(out, eager), it
        assert bool(out[0].isfinite().all()) and bool((out[0] < 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# 4. memory contract
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("misalign", [0, 1, 3])
def test_memory_contract(misalign, dtype):
    for (inshape, shape), window in ((SHAPES[2], [3, 3, 9]), (SHAPES[3], [5, 9, 3]), (SHAPES[4], [9, 9, 9])):
        args = list(cpu.problem(inshape, shape, 400, dtype))
        args[1] = args[1][None]                                          # (the binding takes (B|1, C, *shape))
        for bound, extrapolate in ((3, 1), (6, 0)):
            opt = ([bound] * 3, [3] * 3, extrapolate, "full", window, 1e-3)
            ref = _hip.lcc(*on_device(args), *opt)
            assert all(bool(torch.isfinite(r).all()) for r in ref)
            with memguard.installed(_hip, misalign=misalign) as seam:
                placed = [memguard.place(t, DEV, misalign=misalign) for t in args]
                out = _hip.lcc(*placed, *opt)
                torch.cuda.synchronize()
                what = (shape, bound, misalign)
                assert len(seam.outputs()) == 3 and len(seam.workspaces()) == 1 and seam.workspace_was_written(), what
                assert out[0].shape == (2,) and out[1].shape == (2, *shape, 3) and out[2].shape == (2, *shape, 6), what
                for t in list(out) + placed:
                    assert t.data_ptr() % memguard.ALIGN == misalign * t.element_size(), what
                for t, r in zip(out, ref):
                    seam.assert_fully_written(t, r, what)
                    assert torch.equal(t, r), what
                seam.assert_guards_intact(what)
                for t, a in zip(placed, args):
                    memguard.assert_guard_intact(t, what)
                    assert torch.equal(t.cpu(), a), what


# ---------------------------------------------------------------------------------------------------------------------
# 5. views
# ---------------------------------------------------------------------------------------------------------------------
def raw_call(L, p, moving, fixed, disp, weight, loss, grad, hess, kind, window, eps, wbs, gbs, hbs, ws, nbytes=None):
    ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)
    win = None if window is None else (ctypes.c_int * 3)(*window)
    return L.interpol_lcc(ctypes.byref(p), ptr(moving), ptr(fixed), ptr(disp), ptr(weight), ptr(loss), ptr(grad), ptr(hess), kind,
                          win, eps, wbs, gbs, hbs, ptr(ws), (0 if ws is None else ws.numel()) if nbytes is None else nbytes,
                          ctypes.c_void_p(0))


def workspace_bytes(shape, B, C, es):
    """one double per workgroup (8 x 32 columns, 32 planes; leading extents of 1) and item, three fields of B C N doubles, then one
    of B C N elements"""
    n = [1] * (3 - len(shape)) + list(shape)
    groups = (-(-n[0] // 32)) * (-(-n[1] // 8)) * (-(-n[2] // 32))
    N = n[0] * n[1] * n[2]
    return B * groups * 8 + 3 * B * C * N * 8 + -(-(B * C * N * es) // 8) * 8


@pytest.mark.parametrize("case", [0, 1, 3], ids=[IDS[i] for i in (0, 1, 3)])
def test_views_with_an_offset_strided_channels_and_a_wide_output(case, monkeypatch):
    route_all(monkeypatch)
    inshape, shape = SHAPES[case]
    dim = len(shape)
    moving, fixed, disp, weight = on_device(cpu.problem(inshape, shape, 500 + case, torch.float32))
    fixed = fixed[None]
    window = [5, 3, 9][:dim]
    opt = ([3] * dim, [3] * dim, 1, "full", window, 1e-3)
    ref = _hip.lcc(moving, fixed, disp, weight, *opt)
    buf = torch.full([disp.numel() + 1], float("nan"), device=DEV)
    view = buf[1:].view(disp.shape)
    view.copy_(disp)
    assert view.storage_offset() == 1 and view.data_ptr() % 8 != 0
    big = torch.full([2, 4, *inshape], float("nan"), device=DEV)
    big[:, ::2] = moving
    sliced = big[:, ::2]
    assert sliced.stride(1) == 2 * moving.stride(1) and sliced.data_ptr() == big.data_ptr()
    fperm = fixed.movedim(-1, 1).contiguous().movedim(1, -1)
    dchan = disp.movedim(-1, 1).contiguous().movedim(1, -1)
    for m, f, u in ((moving, fixed, view), (sliced, fixed, disp), (moving, fperm, dchan)):
        assert same(_hip.lcc(m, f, u, weight, *opt), ref), case
        got = interpol.lcc_gauss_newton(m, f, u, weight, interpolation=3, bound="dct2", window=window, eps=1e-3)
        assert same(got, ref), case
    # through the C entry: outputs with a batch stride larger than dense; what lies between the items stays untouched
    L = _hip.lib()
    N, K, pad = disp[0].numel() // dim, dim * (dim + 1) // 2, 5
    p = _hip._ssd_problem(moving, fixed, disp, opt[0], opt[1], 1, 2)
    need = L.interpol_lcc_workspace(ctypes.byref(p))
    assert need == workspace_bytes(shape, 2, 2, 4)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    gbuf = torch.full([2, N * dim + pad], float("nan"), device=DEV)
    hbuf = torch.full([2, N * K + 2 * pad], float("nan"), device=DEV)
    loss = torch.full([2], float("nan"), device=DEV)
    assert raw_call(L, p, moving, fixed, disp, weight, loss, gbuf, hbuf, 2, window + [1] * (3 - dim), 1e-3, weight.stride(0),
                    gbuf.stride(0), hbuf.stride(0), ws) == 0
    torch.cuda.synchronize()
    assert torch.equal(loss, ref[0])
    assert torch.equal(gbuf[:, :N * dim].reshape(ref[1].shape), ref[1]) and bool(gbuf[:, N * dim:].isnan().all())
    assert torch.equal(hbuf[:, :N * K].reshape(ref[2].shape), ref[2]) and bool(hbuf[:, N * K:].isnan().all())


# ---------------------------------------------------------------------------------------------------------------------
# 6. the entry points validate before launching
# ---------------------------------------------------------------------------------------------------------------------
def test_entry_points_validate_before_launching():
    L = _hip.lib()
    inshape, shape = (6, 5, 4), (5, 4, 7)
    N = 5 * 4 * 7
    moving, fixed, disp, weight = on_device(cpu.problem(inshape, shape, 600, torch.float32, C=3))
    fixed = fixed[None].expand(2, *fixed.shape).contiguous()
    sentinel = 4321.0
    loss = torch.full([2], sentinel, device=DEV)
    grad = torch.full([2, *shape, 3], sentinel, device=DEV)
    hess = torch.full([2, *shape, 6], sentinel, device=DEV)

    def problem(dtype=torch.float32, gdtype=None, dim=3, order=(3, 3, 3), bound=3, extrapolate=1, C=3, B=2, mstr=None, dstr=None,
                fstr=None, flags=0, inshp=inshape):
        m = mstr or [moving.stride(0), moving.stride(1), *moving.stride()[2:]]
        d = dstr or [disp.stride(0), *disp.stride()[1:4], 1]
        f = fstr or [fixed.stride(0), fixed.stride(1), *fixed.stride()[2:], 0, 0]
        return _hip.make_problem(dim, dtype, gdtype or dtype, [bound] * 3, list(order), extrapolate, B, C, inshp, shape, m, d, f, flags)

    need = L.interpol_lcc_workspace(ctypes.byref(problem()))
    assert need == workspace_bytes(shape, 2, 3, 4)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)

    def call(p, m=moving, f=fixed, u=disp, w=weight, lo=loss, g=grad, h=hess, kind=2, window=(3, 5, 9), eps=1e-3, wbs=N, gbs=3 * N,
             hbs=6 * N, work=ws, nbytes=None):
        return raw_call(L, p, m, f, u, w, lo, g, h, kind, window, eps, wbs, gbs, hbs, work, nbytes)

    for dim in (0, 4):
        assert call(problem(dim=dim)) == -1 and L.interpol_lcc_workspace(ctypes.byref(problem(dim=dim))) == -1   # INTERPOL_E_DIM
    for order in ((0, 0, 0), (4, 4, 4), (1, 2, 3), (3, 3, 1), (8, 8, 8), (-1, -1, -1)):
        assert call(problem(order=order)) == -2                         # INTERPOL_E_ORDER: one order 1..3
        assert L.interpol_lcc_workspace(ctypes.byref(problem(order=order))) == -2
    for bound in (-1, 7):
        assert call(problem(bound=bound)) == -3                         # INTERPOL_E_BOUND
    for dtype in (torch.bfloat16, torch.float16):
        assert call(problem(dtype=dtype, gdtype=torch.float32)) == -4   # INTERPOL_E_DTYPE
    assert call(problem(gdtype=torch.float64)) == -4
    assert call(problem(C=0)) == -5 and call(problem(B=0)) == -5        # INTERPOL_E_SHAPE
    assert call(problem(inshp=(6, 0, 4))) == -5
    for kind in (-1, 3):
        assert call(problem(), kind=kind) == -5                         # hessian_kind
    for window in ((3, 4, 5), (0, 3, 3), (3, 3, 11), (-1, 3, 3)):
        assert call(problem(), window=window) == -5                     # the window: odd, 1..9
    for eps in (0.0, -1.0, float("nan"), float("inf")):
        assert call(problem(), eps=eps) == -5
    assert call(problem(), window=None) == -6
    for extrapolate in (-1, 3):
        assert call(problem(extrapolate=extrapolate)) == -7             # INTERPOL_E_EXTRAP
    assert call(problem(dstr=[disp.stride(0), 28, 7, 1, N])) == -10     # a channel-first displacement: INTERPOL_E_STRIDE
    assert call(problem(fstr=[fixed.stride(0), 1, 84, 21, 3, 0, 0])) == -10   # a channel-last fixed image
    assert call(problem(mstr=[moving.stride(0), moving.stride(1), -20, 4, 1])) == -10
    assert call(problem(mstr=[-1, moving.stride(1), 20, 4, 1])) == -10
    assert call(problem(flags=_hip.FLAG_SEPARABLE_GRID)) == -10 and call(problem(flags=_hip.FLAG_AFFINE_GRID)) == -10
    assert call(problem(), wbs=-1) == -10 and call(problem(), gbs=-1) == -10 and call(problem(), hbs=-1) == -10
    assert call(problem(), gbs=3 * N - 1) == -10 and call(problem(), hbs=6 * N - 1) == -10    # items of an output that overlap
    assert call(problem(), g=disp) == -10                               # the gradient is the displacement
    assert call(problem(), g=moving.view(-1)[7:]) == -10                # ... starts inside the moving image
    assert call(problem(), h=fixed) == -10 and call(problem(), lo=weight) == -10
    assert call(problem(), h=grad, hbs=3 * N, kind=1) == -10            # two outputs that are one buffer
    assert call(problem(), lo=hess.view(-1)[11:]) == -10
    big = torch.zeros(need + 8, dtype=torch.uint8, device=DEV)
    huge = torch.zeros(need // 4 + 8, device=DEV)                     # (float32: `need` bytes and two elements to spare)
    assert call(problem(), work=huge.view(torch.uint8), g=huge[4:], nbytes=need) == -10   # the workspace overlaps an output
    assert call(problem(), work=huge.view(torch.uint8), u=huge[6:], nbytes=need) == -10   # ... an input
    assert call(problem(), work=big[4:], nbytes=need) == -10            # a workspace that is not 8-byte aligned
    assert call(problem(), nbytes=need - 1) == -9                       # INTERPOL_E_SCRATCH
    for missing in ("m", "f", "u", "lo", "g", "h"):
        assert call(problem(), **{missing: None}) == -6                 # INTERPOL_E_NULL
    assert call(problem(), work=None, nbytes=need) == -6
    assert L.interpol_lcc(None, *[ctypes.c_void_p(0)] * 7, 2, None, 1.0, 0, 0, 0, ctypes.c_void_p(0), 0, ctypes.c_void_p(0)) == -6
    torch.cuda.synchronize()
    assert all(bool((t == sentinel).all()) for t in (loss, grad, hess)) and not bool(ws.any()) and not bool(huge.any())
    # valid calls: a NULL weight, and a NULL Hessian with no Hessian asked for
    ref = _hip.lcc(moving, fixed, disp, weight, [3] * 3, [3] * 3, 1, "full", [3, 5, 9], 1e-3)
    assert call(problem()) == 0
    torch.cuda.synchronize()
    assert torch.equal(loss, ref[0]) and torch.equal(grad, ref[1]) and torch.equal(hess, ref[2]) and bool(ws.any())
    hess.fill_(sentinel)
    assert call(problem(), w=None, h=None, kind=0, wbs=-1, hbs=-1) == 0
    torch.cuda.synchronize()
    assert torch.equal(grad, _hip.lcc(moving, fixed, disp, None, [3] * 3, [3] * 3, 1, None, [3, 5, 9], 1e-3)[1])
    assert bool((hess == sentinel).all())


# ---------------------------------------------------------------------------------------------------------------------
# 7. one Gauss-Newton step on the device, captured as one graph
# ---------------------------------------------------------------------------------------------------------------------
def test_one_gauss_newton_step_on_the_device_as_one_graph(monkeypatch):
    calls = fused_calls(monkeypatch)
    route_all(monkeypatch)
    moving, fixed = cpu.rescaled_blobs(16, 3, torch.float32, DEV)
    disp = torch.zeros(16, 16, 16, 3, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = cpu.gauss_newton_step(moving, fixed, disp)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert calls["lcc"] == 2
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        before, after = cpu.gauss_newton_step(moving, fixed, disp)
    graph.replay()
    torch.cuda.synchronize()
    print("lcc objective on the device %.6g -> %.6g" % (float(before), float(after)))
    assert torch.equal(before, eager[0]) and torch.equal(after, eager[1])
    assert float(after) < float(before) < 0
