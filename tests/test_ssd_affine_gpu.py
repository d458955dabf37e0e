"""`interpol.ssd_gauss_newton_affine` on the device (csrc/ssd_affine.hip).

Truth: the composed form in float64 on the CPU, fed the upcast inputs (tests/test_ssd_affine_cpu.py: `truth_and_allowance`).  The
matrices have dyadic entries (multiples of 1/32), so every coordinate is exact in float32: both sides see the same `floor` and
the same mask, and nothing is masked out or excluded.  (The largest coordinate of these lattices, 0.875 * 299 999 + 2.53125,
takes 19 + 5 bits.)

Allowance per entry: the project's bar applied per sample and summed, from the reference's own per-sample fields --
tol sum_o (|q_d| + max|q_d|) |o~_e| for the gradient, tol sum_o (|h_dd'| + max|h_dd'|) |o~_e o~_e'| for the Hessian,
tol (|ref| + sum_o weight sum_c r_c^2) for the loss; tol = 1e-5 (float32) / 1e-11 (float64).  The float32 bar is loose at large N;
the float64 cases are the ones that catch a dropped or doubled sample.

Lattices (moving -> fixed), each for a way the reduction can go wrong: 1x1x1 and 2x1x1 leave all but one workgroup without a sample;
5x6x7 is a single partial workgroup; 9x33x70 is not a multiple of 256 and leaves most workgroups empty; 40x96x72 has 276 480
samples, more than 1024 * 256, so every workgroup loops; 33x70 and 600x450, 7 and 300 000 are their 2-D and 1-D counterparts.
"""
import ctypes

import pytest
import torch

import interpol
from interpol import _hip, backend, ops
import memguard
import test_ssd_affine_cpu as cpu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = {torch.float32: 1e-5, torch.float64: 1e-11}
F32, F64 = torch.float32, torch.float64
ALL_ORDERS = (1, 2, 3)

# (moving, fixed lattice, dtype, order, bound, extrapolate, C, weighted, hessian)
PARITY = [
    ((3, 2, 2), (1, 1, 1), F64, 1, "dct2", True, 1, False, True),
    ((3, 2, 2), (2, 1, 1), F32, 2, "dft", False, 3, True, True),
    ((7, 5, 6), (5, 6, 7), F64, 3, "zero", False, 3, True, True),
    ((7, 5, 6), (5, 6, 7), F32, 1, "replicate", 2, 1, False, False),
    ((12, 30, 64), (9, 33, 70), F64, 2, "replicate", 2, 1, True, True),
    ((44, 90, 80), (40, 96, 72), F32, 3, "dct2", True, 1, True, True),
    ((44, 90, 80), (40, 96, 72), F64, 1, "dft", False, 1, False, True),
    ((40, 64), (33, 70), F64, 3, "dft", False, 3, True, False),
    ((40, 64), (33, 70), F32, 2, "zero", True, 1, False, True),
    ((512, 512), (600, 450), F32, 1, "dct2", False, 1, True, True),
    ((512, 512), (600, 450), F64, 2, "zero", 2, 1, False, True),
    ((9,), (7,), F64, 3, "replicate", True, 3, True, True),
    ((270000,), (300000,), F32, 2, "dct2", True, 1, False, True),
    ((250000,), (300000,), F64, 1, "zero", False, 1, True, True),
]


def case_id(c):
    return "%s-%s-o%d-%s-e%d-C%d%s%s" % ("x".join(map(str, c[1])), "f32" if c[2] == F32 else "f64", c[3], c[4], int(c[5]), c[6],
                                         "-w" if c[7] else "", "" if c[8] else "-nohess")


def fused_calls(monkeypatch):
    """count the calls that reach the binding of the library"""
    calls = dict(n=0)
    fn = _hip.ssd_affine

    def f(*a, **k):
        calls["n"] += 1
        return fn(*a, **k)

    monkeypatch.setattr(_hip, "ssd_affine", f)
    return calls


def route_all(monkeypatch):
    monkeypatch.setattr(backend, "fused_ssd_affine_orders", ALL_ORDERS)


def dev(t):
    return None if t is None else t.to(DEV)


def same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


def check(got, want, allow, what, hessian=True):
    ratios = dict(loss=cpu.worst_ratio(got[0], want[0], allow[0]), gradient=cpu.worst_ratio(got[1], want[1], allow[1]))
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
    inshape, shape, dtype, order, bound, extrapolate, C, weighted, hessian = case
    route_all(monkeypatch)
    calls = fused_calls(monkeypatch)
    dim = len(shape)
    moving, fixed, weight = cpu.problem(inshape, shape, 1000 + PARITY.index(case), dtype, C=C, B=1, weighted=weighted)
    mat = cpu.matrix(dim, dtype)[None]
    kw = dict(interpolation=order, bound=bound, extrapolate=extrapolate)
    want, allow = cpu.truth_and_allowance(moving, fixed, mat, weight, TOL[dtype], **kw)
    if extrapolate is False and max(shape) > 2:                           # part of the lattice is out of view, part of it in view
        from interpol.sepgrid import AffineGrid
        x = AffineGrid(mat[0].double(), shape).dense()[0]
        inside = ((x > -0.05) & (x < torch.tensor(inshape) - 0.95)).all(-1).double().mean()
        assert 0.0 < float(inside) < 1.0, float(inside)
    got = interpol.ssd_gauss_newton_affine(dev(moving), dev(fixed), dev(mat), dev(weight), hessian=hessian, **kw)
    assert calls["n"] == 1
    P = dim * (dim + 1)
    assert got[0].shape == (1,) and got[1].shape == (1, dim, dim + 1) and (not hessian or got[2].shape == (1, P, P))
    assert all(t.dtype == dtype and t.is_cuda for t in got if t is not None)
    check(got, want, allow, case_id(case), hessian)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_three_matrices_a_shared_moving_image_and_a_batched_weight(dtype, monkeypatch):
    route_all(monkeypatch)
    calls = fused_calls(monkeypatch)
    moving, fixed, weight = cpu.problem((7, 5, 6), (5, 6, 7), 1100, dtype, C=3, B=3)
    mats = torch.stack([cpu.matrix(3, dtype, s) for s in (1.0, 0.5, -0.25)])
    mats[1, 0, 0] += 0.0625
    kw = dict(interpolation=2, bound="dct2", extrapolate=False)
    for m, f, a, w in ((moving[:1], fixed, mats, weight), (moving[:1], fixed[:1], mats[:1], weight), (moving, fixed[:1], mats, None)):
        want, allow = cpu.truth_and_allowance(m, f, a, w, TOL[dtype], **kw)
        got = interpol.ssd_gauss_newton_affine(dev(m), dev(f), dev(a), dev(w), **kw)
        assert got[0].shape == (3,) and got[2].shape == (3, 12, 12)
        check(got, want, allow, "B=3 %s moving %d fixed %d mat %d weight %s" % (dtype, m.shape[0], f.shape[0], a.shape[0], w is not None))
    assert calls["n"] == 3


# ---------------------------------------------------------------------------------------------------------------------
# 2. routing
# ---------------------------------------------------------------------------------------------------------------------
def test_default_routing_reaches_the_fused_kernel_once(monkeypatch):
    calls = fused_calls(monkeypatch)
    assert isinstance(backend.fused_ssd_affine_orders, tuple) and set(backend.fused_ssd_affine_orders) <= set(ALL_ORDERS)
    for (inshape, shape), dtype in ((((7, 5, 6), (5, 6, 7)), F32), (((40, 64), (33, 70)), F64), (((9,), (7,)), F32)):
        dim = len(shape)
        moving, fixed, weight = (dev(t) for t in cpu.problem(inshape, shape, 1200, dtype, B=2))
        mat = dev(cpu.matrix(dim, dtype))
        for order in ALL_ORDERS:
            routed = order in backend.fused_ssd_affine_orders
            assert ops.ssd_affine_covered(moving, fixed, mat[None], weight, [order]) == routed
            before = calls["n"]
            loss, g, h = interpol.ssd_gauss_newton_affine(moving, fixed, mat, weight, interpolation=order)
            assert calls["n"] - before == routed
            assert loss.shape == (2,) and g.shape == (2, dim, dim + 1) and h.shape == (2, dim * (dim + 1), dim * (dim + 1))
            assert all(t.dtype == dtype and t.is_cuda for t in (loss, g, h))


@pytest.mark.parametrize("what", ["bf16", "4d", "mixed_orders", "switched_off"])
def test_uncovered_classes_take_the_composed_route(what, monkeypatch):
    """Each case differs from a call that reaches the fused kernel in ONE property; the control is asserted to reach the binding."""
    route_all(monkeypatch)
    calls = fused_calls(monkeypatch)
    control = [dev(t) for t in cpu.problem((7, 5, 6), (5, 6, 7), 1300, F32)]
    cmat = dev(cpu.matrix(3, F32, 0.25))
    interpol.ssd_gauss_newton_affine(control[0], control[1], cmat, control[2], interpolation=1)
    assert calls["n"] == 1
    order = [1, 2, 3] if what == "mixed_orders" else 1
    if what == "4d":
        gen = torch.Generator().manual_seed(5)
        moving, fixed, weight = torch.randn(2, 3, 4, 3, 4, generator=gen), torch.randn(2, 3, 3, 4, 3, generator=gen), None
        mat = torch.eye(5)[:4] + 0.0625 * torch.randn(4, 5, generator=gen).round()
        order = 1
    else:
        moving, fixed, weight = cpu.problem((7, 5, 6), (5, 6, 7), 1300, torch.bfloat16 if what == "bf16" else F32)
        mat = cpu.matrix(3, moving.dtype, 0.25)
    if what == "switched_off":
        monkeypatch.setattr(backend, "fused_ssd_affine_orders", ())
    kw = dict(interpolation=order, bound="dct2", extrapolate=True)
    got = interpol.ssd_gauss_newton_affine(dev(moving), dev(fixed), dev(mat), dev(weight), **kw)
    assert calls["n"] == 1 and all(t.dtype == moving.dtype and t.is_cuda for t in got)
    want = interpol.ssd_gauss_newton_affine(moving.double(), fixed.double(), mat.double(), None if weight is None else weight.double(), **kw)
    tol = 1e-2 if what == "bf16" else 1e-4                                 # relative to the largest entry: the composed route in float32
    for g, w in zip(got, want):
        assert float((g.double().cpu() - w).abs().max()) <= tol * float(w.abs().max()), what


# ---------------------------------------------------------------------------------------------------------------------
# 3. bits
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_bits_do_not_depend_on_the_run_or_on_the_batch(dtype, monkeypatch):
    route_all(monkeypatch)
    for inshape, shape, order, hessian in (((7, 5, 6), (5, 6, 7), 3, True), ((12, 30, 64), (9, 33, 70), 1, True), ((40, 64), (33, 70), 2, False),
                                           ((9,), (300,), 2, True)):
        dim = len(shape)
        moving, fixed, weight = (dev(t) for t in cpu.problem(inshape, shape, 1400, dtype, B=3))
        mats = dev(torch.stack([cpu.matrix(dim, dtype, s) for s in (1.0, 0.5, -0.25)]))
        kw = dict(interpolation=order, bound="dct2", extrapolate=False, hessian=hessian)
        a = interpol.ssd_gauss_newton_affine(moving, fixed, mats, weight, **kw)
        b = interpol.ssd_gauss_newton_affine(moving, fixed, mats, weight, **kw)
        assert same(a, b), (shape, order)
        if hessian:
            assert torch.equal(a[2], a[2].mT) and bool(a[2].isfinite().all())
        for i in (0, 2):
            one = interpol.ssd_gauss_newton_affine(moving[i], fixed[i], mats[i], weight[i], **kw)
            assert same(one, [None if t is None else t[i] for t in a]), (shape, order, i)


def test_graph_replay_gives_the_bits_of_eager(monkeypatch):
    route_all(monkeypatch)
    moving, fixed, weight = (dev(t) for t in cpu.problem((12, 30, 64), (9, 33, 70), 1500, F32, B=2))
    mat = dev(torch.stack([cpu.matrix(3, F32), cpu.matrix(3, F32, 0.5)]))
    kw = dict(interpolation=3, bound="dct2", extrapolate=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                        # warm-up on the side stream (module loads)
        interpol.ssd_gauss_newton_affine(moving, fixed, mat, weight, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = interpol.ssd_gauss_newton_affine(moving, fixed, mat, weight, **kw)
    for it in range(3):
        mat[:, :, -1] += 0.5 * (it + 1)
        graph.replay()
        torch.cuda.synchronize()
        eager = interpol.ssd_gauss_newton_affine(moving, fixed, mat, weight, **kw)
        assert same(out, eager), it
        assert bool(out[0].isfinite().all()) and bool((out[0] > 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# 4. memory contract
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("misalign", [0, 1, 3])
def test_memory_contract(misalign, dtype):
    for inshape, shape, hessian in (((7, 5, 6), (5, 6, 7), True), ((12, 30, 64), (9, 33, 70), True), ((40, 64), (33, 70), False), ((9,), (7,), True)):
        dim = len(shape)
        moving, fixed, weight = cpu.problem(inshape, shape, 1600, dtype, B=2)
        mat = torch.stack([cpu.matrix(dim, dtype), cpu.matrix(dim, dtype, 0.5)])
        args = [moving, fixed, mat, weight]
        for bound, extrapolate in ((3, 1), (6, 0)):
            opt = ([bound] * 3, [3] * 3, extrapolate, hessian)
            ref = _hip.ssd_affine(*[dev(t) for t in args], *opt)
            assert all(bool(torch.isfinite(r).all()) for r in ref if r is not None)
            with memguard.installed(_hip, misalign=misalign) as seam:
                placed = [memguard.place(t, DEV, misalign=misalign) for t in args]
                out = _hip.ssd_affine(*placed, *opt)
                torch.cuda.synchronize()
                what = (shape, bound, misalign)
                assert len(seam.outputs()) == 2 + hessian and len(seam.workspaces()) == 1 and seam.workspace_was_written(), what
                P = dim * (dim + 1)
                assert out[0].shape == (2,) and out[1].shape == (2, dim, dim + 1) and (not hessian or out[2].shape == (2, P, P)), what
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
# 5. views
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [((7, 5, 6), (5, 6, 7)), ((40, 64), (33, 70)), ((9,), (300,))], ids=["5x6x7", "33x70", "300"])
def test_views_strided_channels_an_offset_image_and_a_row_slice_of_a_square_matrix(case, monkeypatch):
    route_all(monkeypatch)
    calls = fused_calls(monkeypatch)
    inshape, shape = case
    dim = len(shape)
    moving, fixed, weight = (dev(t) for t in cpu.problem(inshape, shape, 1700, F32, B=2))
    mat = dev(torch.stack([cpu.matrix(dim, F32), cpu.matrix(dim, F32, 0.5)]))
    kw = dict(interpolation=3, bound="dct2", extrapolate=True)
    ref = interpol.ssd_gauss_newton_affine(moving, fixed, mat, weight, **kw)
    # a moving image whose storage starts one element into its buffer
    buf = torch.full([moving.numel() + 1], float("nan"), device=DEV)
    view = buf[1:].view(moving.shape)
    view.copy_(moving)
    assert view.storage_offset() == 1 and view.data_ptr() % 8 != 0
    # every other channel of a larger image: a channel stride from slicing, read in place
    big = torch.full([2, 4, *inshape], float("nan"), device=DEV)
    big[:, ::2] = moving
    sliced = big[:, ::2]
    assert sliced.stride(1) == 2 * moving.stride(1) and sliced.data_ptr() == big.data_ptr()
    # the first D rows of (D+1, D+1) matrices: a batch stride of (D+1)^2, read in place
    square = torch.full([2, dim + 1, dim + 1], float("nan"), device=DEV)
    square[:, :dim] = mat
    # fixed / weight that are not row-major: the host makes them dense
    fperm = fixed.movedim(-1, 1).contiguous().movedim(1, -1)
    for m, f, a in ((view, fixed, mat), (sliced, fixed, mat), (moving, fixed, square), (moving, fperm, square[:, :dim])):
        assert same(interpol.ssd_gauss_newton_affine(m, f, a, weight, **kw), ref), case
    assert same(_hip.ssd_affine(moving, fixed, square[:, :dim], weight, [3] * dim, [3] * dim, 1, True), ref)
    assert calls["n"] == 6


# ---------------------------------------------------------------------------------------------------------------------
# 6. the entry points validate before launching
# ---------------------------------------------------------------------------------------------------------------------
def raw_call(L, p, moving, fixed, mat, weight, loss, grad, hess, with_hessian, mbs, wbs, ws, nbytes=None):
    ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)
    return L.interpol_ssd_affine(ctypes.byref(p), ptr(moving), ptr(fixed), ptr(mat), ptr(weight), ptr(loss), ptr(grad), ptr(hess),
                                 with_hessian, mbs, wbs, ptr(ws), (0 if ws is None else ws.numel()) if nbytes is None else nbytes,
                                 ctypes.c_void_p(0))


def test_entry_points_validate_before_launching():
    L = _hip.lib()
    inshape, shape = (6, 5, 4), (5, 4, 7)
    N = 5 * 4 * 7
    moving, fixed, weight = (dev(t) for t in cpu.problem(inshape, shape, 1800, F32, C=3, B=2))
    mat = dev(torch.stack([cpu.matrix(3, F32), cpu.matrix(3, F32, 0.5)]))
    sentinel = 4321.0
    loss = torch.full([2], sentinel, device=DEV)
    grad = torch.full([2, 3, 4], sentinel, device=DEV)
    hess = torch.full([2, 12, 12], sentinel, device=DEV)

    def problem(dtype=F32, gdtype=None, dim=3, order=(3, 3, 3), bound=3, extrapolate=1, C=3, B=2, mstr=None, fstr=None,
                flags=_hip.FLAG_AFFINE_GRID, inshp=inshape, shp=shape):
        m = mstr or [moving.stride(0), moving.stride(1), *moving.stride()[2:]]
        f = fstr or [fixed.stride(0), fixed.stride(1), *fixed.stride()[2:], 0, 0]
        return _hip.make_problem(dim, dtype, gdtype or dtype, [bound] * 3, list(order), extrapolate, B, C, inshp, shp, m, [0] * 5, f, flags)

    need = L.interpol_ssd_affine_workspace(ctypes.byref(problem()))
    assert need == 2 * 73 * 1024 * 8                                    # 73 sums of 1024 workgroups per item
    assert L.interpol_ssd_affine_workspace(ctypes.byref(problem(dim=2, fstr=[0, 0, 4, 1, 0, 0, 0]))) == 2 * 25 * 1024 * 8
    assert L.interpol_ssd_affine_workspace(ctypes.byref(problem(dim=1, fstr=[0, 0, 1, 0, 0, 0, 0]))) == 2 * 6 * 1024 * 8
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)

    def call(p, m=moving, f=fixed, a=mat, w=weight, lo=loss, g=grad, h=hess, wh=1, mbs=12, wbs=N, work=ws, nbytes=None):
        return raw_call(L, p, m, f, a, w, lo, g, h, wh, mbs, wbs, work, nbytes)

    for dim in (0, 4):
        assert call(problem(dim=dim)) == -1 and L.interpol_ssd_affine_workspace(ctypes.byref(problem(dim=dim))) == -1   # INTERPOL_E_DIM
    for order in ((0, 0, 0), (4, 4, 4), (1, 2, 3), (3, 3, 1), (8, 8, 8), (-1, -1, -1)):
        assert call(problem(order=order)) == -2                         # INTERPOL_E_ORDER: one order 1..3
        assert L.interpol_ssd_affine_workspace(ctypes.byref(problem(order=order))) == -2
    for bound in (-1, 7):
        assert call(problem(bound=bound)) == -3                         # INTERPOL_E_BOUND
    for dtype in (torch.bfloat16, torch.float16):
        assert call(problem(dtype=dtype, gdtype=F32)) == -4             # INTERPOL_E_DTYPE
    assert call(problem(gdtype=F64)) == -4 and call(problem(dtype=F64, gdtype=F32)) == -4
    assert call(problem(C=0)) == -5 and call(problem(B=0)) == -5 and call(problem(B=65536)) == -5   # INTERPOL_E_SHAPE
    assert call(problem(inshp=(6, 0, 4))) == -5
    assert call(problem(shp=(1 << 16, 1 << 16, 2), fstr=[0, 0, 1 << 17, 2, 1, 0, 0])) == -5               # 2^33 samples: the sample index is split in 32 bits
    for wh in (-1, 2):
        assert call(problem(), wh=wh) == -5                             # with_hessian
    for extrapolate in (-1, 3):
        assert call(problem(extrapolate=extrapolate)) == -7             # INTERPOL_E_EXTRAP
    assert call(problem(fstr=[fixed.stride(0), 1, 84, 21, 3, 0, 0])) == -10   # a channel-last fixed image: INTERPOL_E_STRIDE
    assert call(problem(mstr=[moving.stride(0), moving.stride(1), -20, 4, 1])) == -10
    assert call(problem(mstr=[-1, moving.stride(1), 20, 4, 1])) == -10
    assert call(problem(fstr=[-1, fixed.stride(1), 28, 7, 1, 0, 0])) == -10
    assert call(problem(flags=_hip.FLAG_SEPARABLE_GRID)) == -10 and call(problem(flags=_hip.FLAG_DISPLACEMENT)) == -10
    assert call(problem(), mbs=-1) == -10 and call(problem(), wbs=-1) == -10
    assert call(problem(), g=mat) == -10                                # the gradient is the matrix
    assert call(problem(), g=moving.view(-1)[7:]) == -10                # ... starts inside the moving image
    assert call(problem(), h=fixed) == -10 and call(problem(), lo=weight) == -10
    assert call(problem(), h=grad.view(-1)) == -10                      # two outputs that overlap
    assert call(problem(), lo=hess.view(-1)[11:]) == -10
    assert call(problem(), work=hess.view(torch.uint8), nbytes=need) == -10           # the workspace is an output
    assert call(problem(), work=moving.view(torch.uint8), nbytes=need) == -10         # ... an input
    big = torch.zeros(need + 8, dtype=torch.uint8, device=DEV)
    assert call(problem(), work=big[4:], nbytes=need) == -10            # a workspace that is not 8-byte aligned
    assert call(problem(), nbytes=need - 1) == -9                       # INTERPOL_E_SCRATCH
    for missing in ("m", "f", "a", "lo", "g", "h"):
        assert call(problem(), **{missing: None}) == -6                 # INTERPOL_E_NULL
    assert call(problem(), work=None, nbytes=need) == -6
    assert L.interpol_ssd_affine(None, *[ctypes.c_void_p(0)] * 7, 1, 0, 0, ctypes.c_void_p(0), 0, ctypes.c_void_p(0)) == -6
    torch.cuda.synchronize()
    assert all(bool((t == sentinel).all()) for t in (loss, grad, hess)) and not bool(ws.any())
    # valid calls: as the binding makes them; a NULL weight and a NULL Hessian with no Hessian asked for
    ref = _hip.ssd_affine(moving, fixed, mat, weight, [3] * 3, [3] * 3, 1, True)
    assert call(problem()) == 0
    torch.cuda.synchronize()
    assert torch.equal(loss, ref[0]) and torch.equal(grad, ref[1]) and torch.equal(hess, ref[2]) and bool(ws.any())
    hess.fill_(sentinel)
    assert call(problem(), w=None, h=None, wh=0, wbs=-1) == 0
    torch.cuda.synchronize()
    assert torch.equal(grad, _hip.ssd_affine(moving, fixed, mat, None, [3] * 3, [3] * 3, 1, False)[1]) and bool((hess == sentinel).all())


# ---------------------------------------------------------------------------------------------------------------------
# 7. recovery of a known matrix on the device
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,order", [(F64, 1), (F64, 3), (F32, 1), (F32, 2), (F32, 3)], ids=["f64-1", "f64-3", "f32-1", "f32-2", "f32-3"])
def test_recovery_of_a_known_matrix(dtype, order, monkeypatch):
    route_all(monkeypatch)
    calls = fused_calls(monkeypatch)
    moving, true = cpu.blobs(dtype, DEV)
    errors = cpu.recover(moving, true, order)
    print("recovery on the device %s order %d: max matrix error per iteration %s" % (dtype, order, " ".join("%.2g" % e for e in errors)))
    assert calls["n"] == 10
    assert errors[-1] <= (1e-8 if dtype == F64 else 1e-4)
