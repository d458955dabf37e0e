"""`interpol.ssd_gauss_newton` on the device (csrc/ssd.hip).

Truth: the composed form evaluated on the CPU in float64 (tests/test_ssd_cpu.py: `reference`), on the inputs as the device sees
them (rounded to its dtype) and at the coordinates o + disp formed in the device's precision, then widened; never the code
under test.  Coordinates within 1e-3 of a spline knot or of a half-integer are moved by 2^-7 before either side sees them
(`nudged`): there a coordinate rounded differently changes the stencil.  Nothing is masked out of the comparison.

Bars: |got - want| <= tol |want| + tol scale, tol = 1e-5 (float32) / 1e-11 (float64); scale = (max|moving| + max|fixed|)
max|moving| max weight for the gradient, max|moving|^2 max weight for the Hessian (not max|want|: on an axis of extent 1 the true
gradient is zero and both sides hold rounding noise), and tol |want| alone for the loss.

Shapes (moving -> fixed): the smallest at which the kernel can go wrong.  (300,) -> (257,) is one sample past a workgroup;
(5, 3, 33) is one past the 4 x 2 x 32 box of a workgroup on every axis; (2, 1) -> (3, 2) and (1, 2, 3) -> (2, 1, 3) have extents
of 1, where every tap wraps.  Under extrapolate = False and sigma = 0.4 at least 40 % of the samples of the four larger shapes
are in view, so the comparison is not zeros against zeros.
"""
import ctypes
import itertools

import pytest
import torch

import interpol
from interpol import _hip, backend, ops
import memguard
import test_ssd_cpu as cpu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = {torch.float32: 1e-5, torch.float64: 1e-11}
SHAPES = [((7,), (5,)), ((300,), (257,)), ((5, 7), (4, 7)), ((2, 1), (3, 2)), ((5, 3, 33), (5, 3, 33)), ((4, 5, 6), (3, 5, 4)),
          ((1, 2, 3), (2, 1, 3))]
TINY = [((7,), (5,)), ((2, 1), (3, 2)), ((1, 2, 3), (2, 1, 3))]
IDS = cpu.IDS(SHAPES)
ALL_ORDERS = (1, 2, 3)


def fused_calls(monkeypatch):
    """count the calls that reach the binding of the library"""
    calls = dict(ssd=0)
    fn = _hip.ssd

    def f(*a, **k):
        calls["ssd"] += 1
        return fn(*a, **k)

    monkeypatch.setattr(_hip, "ssd", f)
    return calls


def route_all(monkeypatch):
    """every order the library instantiates goes to the fused kernel, with and without a Hessian"""
    monkeypatch.setattr(backend, "fused_ssd_orders", ALL_ORDERS)
    monkeypatch.setattr(backend, "fused_ssd_orders_without_hessian", ALL_ORDERS)


def dev(t):
    return None if t is None else t.to(DEV)


def on_device(args):
    return [dev(t) for t in args]


def folded(args):
    """(moving, fixed, disp, weight) as `ops` sees them: `fixed` with its batch of 1"""
    return [args[0], args[1][None], args[2], args[3]]


# ---------------------------------------------------------------------------------------------------------------------
# 1. routing
# ---------------------------------------------------------------------------------------------------------------------
def test_default_routing_reaches_the_fused_kernel_once(monkeypatch):
    calls = fused_calls(monkeypatch)
    assert isinstance(backend.fused_ssd_orders, tuple) and set(backend.fused_ssd_orders) <= set(ALL_ORDERS)
    for (inshape, shape), dtype in itertools.product(SHAPES[1::2] + SHAPES[4:5], (torch.float32, torch.float64)):
        args = on_device(cpu.problem(inshape, shape, 1, dtype))
        for order in backend.fused_ssd_orders:
            assert ops.ssd_covered(*folded(args), [order])
            before = calls["ssd"]
            loss, g, h = interpol.ssd_gauss_newton(*args, interpolation=order)
            assert calls["ssd"] - before == 1
            assert loss.shape == (2,) and g.shape == args[2].shape and h.shape[:-1] == g.shape[:-1]
            assert all(t.dtype == dtype and t.is_cuda for t in (loss, g, h))
    assert set(backend.fused_ssd_orders_without_hessian) <= set(backend.fused_ssd_orders)
    for order in ALL_ORDERS:                                                # without a Hessian: a routing list of its own
        before = calls["ssd"]
        assert interpol.ssd_gauss_newton(*args, interpolation=order, hessian=None)[2] is None
        assert calls["ssd"] - before == (order in backend.fused_ssd_orders_without_hessian)
        assert ops.ssd_covered(*folded(args), [order], None) == (order in backend.fused_ssd_orders_without_hessian)
    assert 1 in backend.fused_ssd_orders                                    # the default call (interpolation=1) is fused
    before = calls["ssd"]
    interpol.ssd_gauss_newton(*on_device(cpu.problem((4, 5, 6), (3, 5, 4), 2, torch.float32)))
    assert calls["ssd"] - before == 1


@pytest.mark.parametrize("what", ["bf16", "4d", "mixed_orders", "switched_off"])
def test_uncovered_classes_take_the_composed_route(what, monkeypatch):
    """Each case differs from a call that reaches the fused kernel in ONE property: order 1 (routed) everywhere but in
    `mixed_orders`, and the control -- the same call without the property -- is asserted to reach the binding."""
    assert 1 in backend.fused_ssd_orders
    inshape, shape = ((3, 2, 4, 3), (2, 3, 3, 2)) if what == "4d" else ((4, 5, 6), (3, 5, 4))
    dtype = torch.bfloat16 if what == "bf16" else torch.float32
    args = cpu.problem(inshape, shape, 3, dtype, sigma=0.7)
    order = [1, 2, 3] if what == "mixed_orders" else 1
    kw = dict(interpolation=order, bound="dct2", extrapolate=True)
    calls = fused_calls(monkeypatch)
    # the control: float32, three dimensions, order 1, the switch as it is
    control = cpu.problem((4, 5, 6), (3, 5, 4), 3, torch.float32, sigma=0.7) if what == "4d" else [t.float() for t in args]
    assert ops.ssd_covered(*folded(on_device(control)), [1])
    interpol.ssd_gauss_newton(*on_device(control), **dict(kw, interpolation=1))
    assert calls["ssd"] == 1
    if what == "switched_off":
        monkeypatch.setattr(backend, "fused_ssd_orders", ())
    assert not ops.ssd_covered(*folded(on_device(args)), order if isinstance(order, list) else [order])
    got = interpol.ssd_gauss_newton(*on_device(args), **kw)
    assert calls["ssd"] == 1 and all(t.dtype == dtype and t.is_cuda for t in got)
    want = cpu.reference(*[t.float() for t in args], **kw)               # (the coordinates are formed in float32 on the device)
    sg, sh = cpu.scales(*[args[i] for i in (0, 1, 3)])
    tol = 1e-2 if what == "bf16" else TOL[torch.float32]
    # (16-bit: one rounding of each output on top of the float32 error; the coordinates are the rounded displacements' on both sides)
    assert cpu.ratio(got[0], want[0], tol, 0.0) <= 1.0
    assert cpu.ratio(got[1], want[1], tol, sg) <= 1.0 and cpu.ratio(got[2], want[2], tol, sh) <= 1.0


def test_only_the_weight_carries_the_batch(monkeypatch):
    """moving, fixed and disp without a batch, weight with one: both routes give one item per weight"""
    calls = fused_calls(monkeypatch)
    moving, fixed, disp, weight = cpu.problem((4, 5, 6), (3, 5, 4), 4, torch.float32, sigma=0.7)
    kw = dict(interpolation=1, bound="dct2", extrapolate=False)
    want = cpu.reference(moving[0], fixed, disp[0], weight, **kw)
    sg, sh = cpu.scales(moving, fixed, weight)
    for route in ("fused", "composed"):
        if route == "composed":
            monkeypatch.setattr(backend, "fused_ssd_orders", ())
        got = interpol.ssd_gauss_newton(dev(moving[0]), dev(fixed), dev(disp[0]), dev(weight), **kw)
        assert calls["ssd"] == 1 and got[0].shape == (2,) and got[1].shape == disp.shape and got[2].shape == (2, 3, 5, 4, 6)
        assert cpu.ratio(got[0], want[0], 1e-5, 0.0) <= 1.0 and cpu.ratio(got[1], want[1], 1e-5, sg) <= 1.0
        assert cpu.ratio(got[2], want[2], 1e-5, sh) <= 1.0


def test_extrapolate_2_is_the_mask_of_pull_and_grad():
    """the binding at extrapolate = 2 (a lattice half a voxel wider is in view) against interpol_pull / interpol_grad with it"""
    seen = {0: 0, 2: 0}
    for inshape, shape, order in (((4, 5, 6), (3, 5, 4), 3), ((5, 7), (4, 7), 2), ((7,), (5,), 1)):
        dim = len(shape)
        moving, fixed, disp, weight = on_device(cpu.problem(inshape, shape, 5, torch.float32, sigma=2.0))
        disp, _ = cpu.nudged(disp.cpu(), order)
        disp, fixed = disp.to(DEV), fixed[None]
        out = {}
        for extrapolate in (0, 2):
            opt = ([3] * dim, [order] * dim, extrapolate)
            loss, g, h = _hip.ssd(moving, fixed, disp, weight, *opt, "full")
            w = _hip.gather("pull", moving, disp, *opt, flags=_hip.FLAG_DISPLACEMENT)
            G = _hip.gather("grad", moving, disp, *opt, flags=_hip.FLAG_DISPLACEMENT)
            r = (w - fixed).double()
            wt, G = weight.double(), G.double()
            sg, sh = cpu.scales(moving, fixed, weight)
            assert cpu.ratio(loss, 0.5 * (wt.unsqueeze(1) * r * r).flatten(1).sum(1).cpu(), 1e-5, 0.0) <= 1.0
            assert cpu.ratio(g, ((G * r.unsqueeze(-1)).sum(1) * wt.unsqueeze(-1)).cpu(), 1e-5, sg) <= 1.0
            want_h = torch.stack([(G[..., d] * G[..., e]).sum(1) for d, e in
                                  [(d, d) for d in range(dim)] + [(d, e) for d in range(dim) for e in range(d + 1, dim)]], -1)
            assert cpu.ratio(h, (want_h * wt.unsqueeze(-1)).cpu(), 1e-5, sh) <= 1.0
            out[extrapolate] = (g != 0).any(-1)
        # the wider view keeps every sample of the narrower one
        assert bool((out[2] | ~out[0]).all()), shape
        seen[0] += int(out[0].sum())
        seen[2] += int(out[2].sum())
    assert seen[2] > seen[0] > 0, seen                                   # ... and, under these fields, some more


# ---------------------------------------------------------------------------------------------------------------------
# 2. parity with the composed form in float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", range(len(SHAPES)), ids=IDS)
def test_parity_with_the_composed_form_in_float64(case, dtype, monkeypatch):
    inshape, shape = SHAPES[case]
    route_all(monkeypatch)
    calls = fused_calls(monkeypatch)
    tol = TOL[dtype]
    worst = dict(loss=0.0, gradient=0.0, hessian=0.0)
    moved, n_calls = [], 0
    for n, (order, bound, extrapolate) in enumerate(itertools.product(ALL_ORDERS, cpu.BOUNDS, (False, True))):
        C, weighted = (1, 3)[n % 2], (n // 2) % 2 == 1
        for sigma in (2.0, 0.4):
            moving, fixed, disp, weight = cpu.problem(inshape, shape, 1000 * case + 2 * n + (sigma < 1), dtype, C=C, sigma=sigma,
                                                      weighted=weighted)
            disp, frac = cpu.nudged(disp, order)
            moved.append(frac)
            if not extrapolate and sigma < 1 and (inshape, shape) not in TINY:
                assert cpu.in_view(disp, inshape) >= 0.40, (inshape, shape, n)
            kw = dict(interpolation=order, bound=bound, extrapolate=extrapolate)
            want = cpu.reference(moving, fixed, disp, weight, hessian="full", **kw)
            sg, sh = cpu.scales(moving, fixed, weight)
            kinds = ("full", "diagonal", None) if n == 3 * len(shape) else ("full",)
            for kind in kinds:
                got = interpol.ssd_gauss_newton(dev(moving), dev(fixed), dev(disp), dev(weight), hessian=kind, **kw)
                n_calls += 1
                assert got[0].shape == (2,) and got[1].shape == disp.shape and all(t.dtype == dtype for t in got if t is not None)
                ratios = dict(loss=cpu.ratio(got[0], want[0], tol, 0.0), gradient=cpu.ratio(got[1], want[1], tol, sg))
                if kind is None:
                    assert got[2] is None
                else:
                    K = len(shape) if kind == "diagonal" else want[2].shape[-1]
                    assert got[2].shape == (2, *shape, K)
                    ratios["hessian"] = cpu.ratio(got[2], want[2][..., :K], tol, sh)
                for k, v in ratios.items():
                    worst[k] = max(worst[k], v)
                print("parity %s->%s %s order %d %s extrapolate %d C %d weight %d sigma %.1f %s: error / bar %s"
                      % (inshape, shape, dtype, order, bound, extrapolate, C, weighted, sigma, kind,
                         ", ".join("%s %.3g" % kv for kv in ratios.items())))
                assert all(v <= 1.0 for v in ratios.values()), (inshape, shape, dtype, kw, C, weighted, sigma, kind, ratios)
    print("parity %s->%s %s: worst error / bar: loss %.3g, gradient %.3g, hessian %.3g; %.2f %% of the coordinates nudged"
          % (inshape, shape, dtype, worst["loss"], worst["gradient"], worst["hessian"], 100 * sum(moved) / len(moved)))
    assert calls["ssd"] == n_calls


# ---------------------------------------------------------------------------------------------------------------------
# 3. bits
# ---------------------------------------------------------------------------------------------------------------------
def same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_bits_do_not_depend_on_the_run_or_on_the_batch(dtype, monkeypatch):
    route_all(monkeypatch)
    for ((inshape, shape), order, kind) in ((SHAPES[4], 3, "full"), (SHAPES[1], 2, "diagonal"), (SHAPES[2], 1, None), (SHAPES[5], 1, "full")):
        moving, fixed, disp, weight = on_device(cpu.problem(inshape, shape, 40, dtype, B=3))
        fixed = fixed[None].expand(3, *fixed.shape).contiguous()
        kw = dict(interpolation=order, bound="dct2", extrapolate=False, hessian=kind)
        a = interpol.ssd_gauss_newton(moving, fixed, disp, weight, **kw)
        b = interpol.ssd_gauss_newton(moving, fixed, disp, weight, **kw)
        assert same(a, b), (shape, order)
        one = interpol.ssd_gauss_newton(moving[:1], fixed[:1], disp[:1], weight[:1], **kw)
        assert same([None if t is None else t[0] for t in one], [None if t is None else t[0] for t in a]), (shape, order)


# (slots per item, length of the 1-D lattice): the finish (csrc/data_term.hpp: slot_finish) adds rounds of FINISH_WAYS * BLOCK = 2048
# slots, a thread takes a whole round while its slot 1792 further on exists, and what is left goes through the partial round
FINISH_EDGES = [(1, 37), (1792, 1792 * 256 - 5), (1793, 1792 * 256 + 1), (2048, 2048 * 256 - 3), (2049, 2048 * 256 + 1), (4097, 4096 * 256 + 1)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("slots,n", FINISH_EDGES, ids=[str(s) for s, _ in FINISH_EDGES])
def test_the_finish_at_the_edges_of_its_rounds(slots, n, dtype, monkeypatch):
    """fewer slots than one round, whole rounds and a partial last round: the loss against the composed form in float64 (linear,
    where the loss is continuous in the coordinate: nothing is nudged), and each of two items to the bits it gives alone"""
    route_all(monkeypatch)
    calls = fused_calls(monkeypatch)
    moving, fixed, disp, weight = cpu.problem((n,), (n,), 7000 + slots, dtype, C=1)
    kw = dict(interpolation=1, bound="dct2", extrapolate=True, hessian=None)
    want = cpu.reference(moving, fixed, disp, weight, **kw)
    moving, fixed, disp, weight = on_device((moving, fixed, disp, weight))
    p = _hip._ssd_problem(moving, fixed[None], disp, [3], [1], 1, 2)
    need = _hip.lib().interpol_ssd_workspace(ctypes.byref(p))
    assert need == 2 * 8 * slots                                         # (the case has not drifted off its edge)
    both = interpol.ssd_gauss_newton(moving, fixed, disp, weight, **kw)
    ratio = cpu.ratio(both[0], want[0], TOL[dtype], 0.0)
    print("finish %d slots %s: loss error / bar %.3g" % (slots, dtype, ratio))
    assert ratio <= 1.0
    for b in range(2):
        one = interpol.ssd_gauss_newton(moving[b:b + 1], fixed, disp[b:b + 1], weight[b:b + 1], **kw)
        assert torch.equal(one[0][0], both[0][b]) and torch.equal(one[1][0], both[1][b]), (slots, b)
    assert calls["ssd"] == 3


def test_graph_replay_gives_the_bits_of_eager(monkeypatch):
    route_all(monkeypatch)
    inshape, shape = SHAPES[4]
    moving, fixed, disp, weight = on_device(cpu.problem(inshape, shape, 50, torch.float32))
    kw = dict(interpolation=3, bound="dct2", extrapolate=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                        # warm-up on the side stream (module loads)
        interpol.ssd_gauss_newton(moving, fixed, disp, weight, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = interpol.ssd_gauss_newton(moving, fixed, disp, weight, **kw)
    gen = torch.Generator().manual_seed(51)
    for it in range(3):
        disp.copy_(torch.randn(disp.shape, generator=gen) * (1 + it))
        graph.replay()
        torch.cuda.synchronize()
        eager = interpol.ssd_gauss_newton(moving, fixed, disp, weight, **kw)
        assert same(out, eager), it
        assert bool(out[0].isfinite().all()) and bool((out[0] > 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# 4. memory contract
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("misalign", [0, 1, 3])
def test_memory_contract(misalign, dtype):
    for inshape, shape in (SHAPES[4], SHAPES[5], SHAPES[6]):
        args = list(cpu.problem(inshape, shape, 400, dtype))
        args[1] = args[1][None]                                          # (the binding takes (B|1, C, *shape))
        for bound, extrapolate in ((3, 1), (6, 0)):
            opt = ([bound] * 3, [3] * 3, extrapolate, "full")
            ref = _hip.ssd(*on_device(args), *opt)
            assert all(bool(torch.isfinite(r).all()) for r in ref)
            with memguard.installed(_hip, misalign=misalign) as seam:
                placed = [memguard.place(t, DEV, misalign=misalign) for t in args]
                out = _hip.ssd(*placed, *opt)
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
def raw_call(L, p, moving, fixed, disp, weight, loss, grad, hess, kind, wbs, gbs, hbs, ws, nbytes=None):
    ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)
    return L.interpol_ssd(ctypes.byref(p), ptr(moving), ptr(fixed), ptr(disp), ptr(weight), ptr(loss), ptr(grad), ptr(hess), kind,
                          wbs, gbs, hbs, ptr(ws), (0 if ws is None else ws.numel()) if nbytes is None else nbytes, ctypes.c_void_p(0))


@pytest.mark.parametrize("case", [1, 2, 4], ids=[IDS[i] for i in (1, 2, 4)])
def test_views_with_an_offset_strided_channels_and_a_wide_output(case, monkeypatch):
    route_all(monkeypatch)
    inshape, shape = SHAPES[case]
    dim = len(shape)
    moving, fixed, disp, weight = on_device(cpu.problem(inshape, shape, 500 + case, torch.float32))
    fixed = fixed[None]                                                  # (the binding takes (B|1, C, *shape))
    opt = ([3] * dim, [3] * dim, 1, "full")
    ref = _hip.ssd(moving, fixed, disp, weight, *opt)
    # a displacement field whose storage starts one element into its buffer
    buf = torch.full([disp.numel() + 1], float("nan"), device=DEV)
    view = buf[1:].view(disp.shape)
    view.copy_(disp)
    assert view.storage_offset() == 1 and view.data_ptr() % 8 != 0
    # every other channel of a larger image: a channel stride from slicing, read in place
    big = torch.full([2, 6, *inshape], float("nan"), device=DEV)
    big[:, ::2] = moving
    sliced = big[:, ::2]
    assert sliced.stride(1) == 2 * moving.stride(1) and sliced.data_ptr() == big.data_ptr()
    # fixed / weight that are not row-major, disp stored channel-first: the host makes them dense
    fperm = fixed.movedim(-1, 1).contiguous().movedim(1, -1)
    dchan = disp.movedim(-1, 1).contiguous().movedim(1, -1)
    for m, f, u in ((moving, fixed, view), (sliced, fixed, disp), (moving, fperm, dchan)):
        assert cpu_same(_hip.ssd(m, f, u, weight, *opt), ref), case
        got = interpol.ssd_gauss_newton(m, f, u, weight, interpolation=3, bound="dct2")
        assert cpu_same(got, ref), case
    # through the C entry: outputs with a batch stride larger than dense; what lies between the items stays untouched
    L = _hip.lib()
    N, K, pad = disp[0].numel() // dim, dim * (dim + 1) // 2, 5
    p = _hip._ssd_problem(moving, fixed, disp, opt[0], opt[1], 1, 2)
    need = L.interpol_ssd_workspace(ctypes.byref(p))
    assert need == 2 * 8 * (-(-N // 256) if dim < 3 else (-(-shape[0] // 4)) * (-(-shape[1] // 2)) * (-(-shape[2] // 32)))
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    gbuf = torch.full([2, N * dim + pad], float("nan"), device=DEV)
    hbuf = torch.full([2, N * K + 2 * pad], float("nan"), device=DEV)
    loss = torch.full([2], float("nan"), device=DEV)
    assert raw_call(L, p, moving, fixed, disp, weight, loss, gbuf, hbuf, 2, weight.stride(0), gbuf.stride(0), hbuf.stride(0), ws) == 0
    torch.cuda.synchronize()
    assert torch.equal(loss, ref[0])
    assert torch.equal(gbuf[:, :N * dim].reshape(ref[1].shape), ref[1]) and bool(gbuf[:, N * dim:].isnan().all())
    assert torch.equal(hbuf[:, :N * K].reshape(ref[2].shape), ref[2]) and bool(hbuf[:, N * K:].isnan().all())


def cpu_same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------------
# 6. the entry points validate before launching
# ---------------------------------------------------------------------------------------------------------------------
def test_entry_points_validate_before_launching():
    L = _hip.lib()
    inshape, shape = (6, 5, 4), (5, 4, 7)
    N = 5 * 4 * 7
    moving, fixed, disp, weight = on_device(cpu.problem(inshape, shape, 600, torch.float32))
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

    need = L.interpol_ssd_workspace(ctypes.byref(problem()))
    assert need == 2 * 2 * 2 * 1 * 8                                    # one double per 4 x 2 x 32 box and item
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)

    def call(p, m=moving, f=fixed, u=disp, w=weight, lo=loss, g=grad, h=hess, kind=2, wbs=N, gbs=3 * N, hbs=6 * N, work=ws, nbytes=None):
        return raw_call(L, p, m, f, u, w, lo, g, h, kind, wbs, gbs, hbs, work, nbytes)

    for dim in (0, 4):
        assert call(problem(dim=dim)) == -1 and L.interpol_ssd_workspace(ctypes.byref(problem(dim=dim))) == -1   # INTERPOL_E_DIM
    for order in ((0, 0, 0), (4, 4, 4), (1, 2, 3), (3, 3, 1), (8, 8, 8), (-1, -1, -1)):
        assert call(problem(order=order)) == -2                         # INTERPOL_E_ORDER: one order 1..3
        assert L.interpol_ssd_workspace(ctypes.byref(problem(order=order))) == -2
    for bound in (-1, 7):
        assert call(problem(bound=bound)) == -3                         # INTERPOL_E_BOUND
    for dtype in (torch.bfloat16, torch.float16):
        assert call(problem(dtype=dtype, gdtype=torch.float32)) == -4   # INTERPOL_E_DTYPE
    assert call(problem(gdtype=torch.float64)) == -4
    assert call(problem(dtype=torch.float64, gdtype=torch.float32)) == -4
    assert call(problem(C=0)) == -5 and call(problem(B=0)) == -5        # INTERPOL_E_SHAPE
    assert call(problem(inshp=(6, 0, 4))) == -5
    for kind in (-1, 3):
        assert call(problem(), kind=kind) == -5                         # hessian_kind
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
    assert call(problem(), work=grad.view(torch.uint8), nbytes=need) == -10           # the workspace is an output
    assert call(problem(), work=disp.view(torch.uint8), nbytes=need) == -10           # ... an input
    big = torch.zeros(need + 8, dtype=torch.uint8, device=DEV)
    assert call(problem(), work=big[4:], nbytes=need) == -10            # a workspace that is not 8-byte aligned
    assert call(problem(), nbytes=need - 1) == -9                       # INTERPOL_E_SCRATCH
    for missing in ("m", "f", "u", "lo", "g", "h"):
        assert call(problem(), **{missing: None}) == -6                 # INTERPOL_E_NULL
    assert call(problem(), work=None, nbytes=need) == -6
    assert L.interpol_ssd(None, *[ctypes.c_void_p(0)] * 7, 2, 0, 0, 0, ctypes.c_void_p(0), 0, ctypes.c_void_p(0)) == -6
    torch.cuda.synchronize()
    assert all(bool((t == sentinel).all()) for t in (loss, grad, hess)) and not bool(ws.any())
    # valid calls: a NULL weight, and a NULL Hessian with no Hessian asked for
    ref = _hip.ssd(moving, fixed, disp, weight, [3] * 3, [3] * 3, 1, "full")
    assert call(problem()) == 0
    torch.cuda.synchronize()
    assert torch.equal(loss, ref[0]) and torch.equal(grad, ref[1]) and torch.equal(hess, ref[2]) and bool(ws.any())
    hess.fill_(sentinel)
    assert call(problem(), w=None, h=None, kind=0, wbs=-1, hbs=-1) == 0
    torch.cuda.synchronize()
    assert torch.equal(grad, _hip.ssd(moving, fixed, disp, None, [3] * 3, [3] * 3, 1, None)[1]) and bool((hess == sentinel).all())


# ---------------------------------------------------------------------------------------------------------------------
# 7. one Gauss-Newton step on the device, captured as one graph
# ---------------------------------------------------------------------------------------------------------------------
def test_one_gauss_newton_step_on_the_device_as_one_graph(monkeypatch):
    calls = fused_calls(monkeypatch)
    route_all(monkeypatch)
    moving, fixed = cpu.blobs(16, 3, torch.float32, DEV)
    disp = torch.zeros(16, 16, 16, 3, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = cpu.gauss_newton_step(moving, fixed, disp)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert calls["ssd"] == 2
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        before, after = cpu.gauss_newton_step(moving, fixed, disp)
    graph.replay()
    torch.cuda.synchronize()
    print("objective on the device %.6g -> %.6g" % (float(before), float(after)))
    assert torch.equal(before, eager[0]) and torch.equal(after, eager[1])
    assert float(before) > 0 and float(after) < float(before)
