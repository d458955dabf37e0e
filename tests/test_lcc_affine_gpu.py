"""`interpol.lcc_gauss_newton_affine` on the device (csrc/lcc_affine.hip).

Truth: `test_lcc_cpu.truth` in float64 on the upcast inputs at the dense lattice of the dyadic matrices `test_ssd_affine_cpu.matrix`,
contracted in float64 (tests/test_lcc_affine_cpu.py: `dense_truth`).  Every coordinate is exact in float32, so both sides see the
same `floor` and the same mask: nothing is nudged or masked.

Allowance per entry (`truth_and_allowance`): the project's bar applied per sample and summed, from the truth's own per-sample fields --
tol sum_o (|q_d| + max|q_d|) |o~_e| for the gradient, likewise with the moments for the Hessian, tol |want| for the loss; tol = 1e-5
(float32) / 1e-11 (float64).  The float32 rounding of I and G alone, emulated on the CPU, moves the three outputs by at most 0.07 of
this allowance: the float32 bar is loose, the float64 cases are the ones that catch a dropped or doubled sample, and every lattice
has one.  The groups of (offset, eps) are the three that tests/test_lcc_gpu.py compares: (0, 1e-5), (0, 1), (10, 1).

Lattices (moving -> fixed), each for a way the march or the sums can go wrong: (1,2,3) -> (2,1,3) has extents of 1 and a window that
swallows an axis (extrapolate=True only: none of its samples is in view; order 1 only: along the moving extent of 1 the truth's G_0
is identically zero, so the allowance of that row of the gradient and of the Hessian is zero -- the linear derivative weights -1, +1
cancel exactly in every precision, while those of orders 2 and 3 sum to zero only to rounding, 1e-7 of the image in float32, which
an allowance built from a zero field cannot admit; the cubic float32 case first chosen here stood at 2e13 for that reason); (7,5,6) -> (5,6,7) is a single partial workgroup of the
sums; (30,8,35) -> (33,9,33) is one past the 8 x 32 tile and the chunk of 32 planes on every axis; (10,9,40) -> (9,10,36);
(44,90,80) -> (40,96,72) has 276 480 samples, more than 1024 x 256, so every workgroup of the sums loops (window 5); 2-D: (9,12) ->
(8,13), (40,64) -> (9,33), (512,512) -> (600,450); 1-D: (200,) -> (257,), (270000,) -> (300000,).  Every `extrapolate=False` case
asserts that between 40 % and under 100 % of its samples are in view.

Worst error / allowance as measured on an MI355X (profiles/lcc_affine.txt holds the lines per case):
loss / gradient / Hessian, worst over the cases of a group:
  float32, (offset, eps) = (0, 1e-5): loss 0.0029, gradient 0.00022, hessian 0.00027
  float32, (offset, eps) = (0, 1): loss 0.0045, gradient 0.0018, hessian 0.0087
  float32, (offset, eps) = (10, 1): loss 0.069, gradient 0.0012, hessian 0.0018
  float64, (offset, eps) = (0, 1e-5): loss 2.5e-05, gradient 7.2e-06, hessian 3.9e-05
  float64, (offset, eps) = (0, 1): loss 2.4e-05, gradient 9e-07, hessian 3.1e-06
  float64, (offset, eps) = (10, 1): loss 0.00032, gradient 9.2e-05, hessian 0.00023
and over the batches of 65 538 items: float32 0.076 / 0.096 / 0.058, float64 7.2e-4 / 0.017 / 0.011.
"""
import ctypes

import pytest
import torch

import interpol
from interpol import _hip, backend, ops
import batch_loops as BL
import memguard
import test_lcc_affine_cpu as cpu
import test_lcc_cpu as lcc
import test_ssd_affine_cpu as aff

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = {torch.float32: 1e-5, torch.float64: 1e-11}
F32, F64 = torch.float32, torch.float64
ALL_ORDERS = (1, 2, 3)
GROUPS = ((0.0, 1e-5), (0.0, 1.0), (10.0, 1.0))                        # (offset, eps)

# (moving, fixed lattice, dtype, order, bound, extrapolate, C, weighted, hessian, window, group, scale of the translation)
PARITY = [
    ((1, 2, 3), (2, 1, 3), F64, 1, "dct2", True, 1, False, True, 3, 0, 1.0),
    ((1, 2, 3), (2, 1, 3), F32, 1, "dft", True, 3, True, True, [3, 9, 5], 1, 1.0),
    ((7, 5, 6), (5, 6, 7), F64, 3, "zero", True, 3, True, True, 3, 0, 1.0),
    ((7, 5, 6), (5, 6, 7), F32, 3, "replicate", True, 1, False, False, 9, 2, 1.0),
    ((30, 8, 35), (33, 9, 33), F64, 2, "replicate", False, 1, True, True, 5, 1, 1.0),
    ((30, 8, 35), (33, 9, 33), F32, 3, "dct2", True, 3, False, True, 9, 1, 1.0),
    ((10, 9, 40), (9, 10, 36), F64, 1, "dft", False, 3, False, True, [3, 9, 5], 2, 1.0),
    ((10, 9, 40), (9, 10, 36), F32, 2, "zero", False, 1, True, False, [5, 1, 3], 0, 1.0),
    ((44, 90, 80), (40, 96, 72), F32, 3, "dct2", True, 1, True, True, 5, 1, 1.0),
    ((44, 90, 80), (40, 96, 72), F64, 1, "dft", False, 1, False, True, 5, 0, 1.0),
    ((9, 12), (8, 13), F64, 3, "dft", False, 3, True, True, [3, 9], 0, 1.0),
    ((9, 12), (8, 13), F32, 1, "zero", True, 1, False, True, 5, 2, 1.0),
    ((40, 64), (9, 33), F64, 2, "dct2", False, 1, False, False, 9, 1, 1.0),
    ((40, 64), (9, 33), F32, 3, "replicate", True, 3, True, True, [1, 5], 0, 1.0),
    ((512, 512), (600, 450), F32, 1, "dct2", False, 1, True, True, 9, 1, 1.0),
    ((512, 512), (600, 450), F64, 2, "zero", True, 1, False, True, 3, 2, 1.0),
    ((200,), (257,), F64, 3, "replicate", False, 3, True, True, 9, 0, 1.0),
    ((200,), (257,), F32, 2, "dft", True, 1, False, True, 5, 1, 1.0),
    ((270000,), (300000,), F32, 2, "dct2", True, 1, False, True, 3, 1, 1.0),
    ((270000,), (300000,), F64, 1, "zero", False, 1, True, True, 9, 0, 4096.0),    # (t = 10368: the last 1.1 % leave the view)
]


def case_id(c):
    win = "x".join(map(str, c[9])) if isinstance(c[9], list) else str(c[9])
    return "%s-%s-o%d-%s-e%d-C%d%s%s-w%s-g%d" % ("x".join(map(str, c[1])), "f32" if c[2] == F32 else "f64", c[3], c[4], int(c[5]), c[6],
                                                 "-w" if c[7] else "", "" if c[8] else "-nohess", win, c[10])


def fused_calls(monkeypatch):
    """count the calls that reach the binding of the library"""
    calls = dict(n=0)
    fn = _hip.lcc_affine

    def f(*a, **k):
        calls["n"] += 1
        return fn(*a, **k)

    monkeypatch.setattr(_hip, "lcc_affine", f)
    return calls


def route_all(monkeypatch):
    monkeypatch.setattr(backend, "fused_lcc_affine_orders", ALL_ORDERS)


def dev(t):
    return None if t is None else t.to(DEV)


def same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


def images(inshape, shape, seed, dtype, C=2, B=1, weighted=True, offset=0.0):
    """`test_lcc_cpu.problem` without its displacements, as the kernel table takes them: moving (B,C,*in), fixed (1,C,*shape),
    weight (B,*shape) | None"""
    moving, fixed, _, weight = lcc.problem(inshape, shape, seed, dtype, C=C, B=B, weighted=weighted, offset=offset)
    return moving, fixed[None], weight


def in_view(mat, inshape, shape):
    """fraction of the samples that `extrapolate=False` keeps: every coordinate in (-0.05, n - 1 + 0.05)"""
    dim = len(shape)
    o = torch.stack(torch.meshgrid(*[torch.arange(n, dtype=F64) for n in shape], indexing="ij"), -1)
    a = mat.double().cpu().reshape([-1] + [1] * dim + [dim, dim + 1])
    x = (a[..., :dim] * o.unsqueeze(-2)).sum(-1) + a[..., dim]
    ok = torch.ones(x.shape[:-1], dtype=torch.bool)
    for d, n in enumerate(inshape):
        ok &= (x[..., d] > -0.05) & (x[..., d] < n - 1 + 0.05)
    return float(ok.double().mean())


def check(got, want, allow, what, hessian=True):
    ratios = dict(loss=aff.worst_ratio(got[0], want[0], allow[0]), gradient=aff.worst_ratio(got[1], want[1], allow[1]))
    if hessian:
        ratios["hessian"] = aff.worst_ratio(got[2], want[2], allow[2])
        assert torch.equal(got[2], got[2].mT), what
    else:
        assert got[2] is None, what
    print("LCCAFFINE parity %s: worst error / allowance: %s" % (what, ", ".join("%s %.3g" % kv for kv in ratios.items())))
    assert all(v <= 1.0 for v in ratios.values()), (what, ratios)
    return ratios


# ---------------------------------------------------------------------------------------------------------------------
# 1. parity with the definition in float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PARITY, ids=case_id)
def test_parity_with_the_definition_in_float64(case, monkeypatch):
    inshape, shape, dtype, order, bound, extrapolate, C, weighted, hessian, window, group, scale = case
    route_all(monkeypatch)
    calls = fused_calls(monkeypatch)
    dim = len(shape)
    offset, eps = GROUPS[group]
    moving, fixed, weight = images(inshape, shape, 2000 + PARITY.index(case), dtype, C=C, weighted=weighted, offset=offset)
    mat = aff.matrix(dim, dtype, scale)[None]
    kw = dict(interpolation=order, bound=bound, extrapolate=extrapolate)
    if not extrapolate:                                                  # part of the lattice is out of view, most of it in view
        inside = in_view(mat, inshape, shape)
        assert 0.40 <= inside < 1.0, inside
    want, allow = cpu.truth_and_allowance(moving, fixed, mat, weight, TOL[dtype], window, eps, **kw)
    got = interpol.lcc_gauss_newton_affine(dev(moving), dev(fixed), dev(mat), dev(weight), window=window, eps=eps, hessian=hessian, **kw)
    assert calls["n"] == 1
    P = dim * (dim + 1)
    assert got[0].shape == (1,) and got[1].shape == (1, dim, dim + 1) and (not hessian or got[2].shape == (1, P, P))
    assert all(t.dtype == dtype and t.is_cuda for t in got if t is not None)
    check(got, want, allow, case_id(case), hessian)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_three_matrices_a_shared_moving_image_and_a_batched_weight(dtype, monkeypatch):
    route_all(monkeypatch)
    calls = fused_calls(monkeypatch)
    moving, fixed, weight = images((7, 5, 6), (5, 6, 7), 2100, dtype, C=3, B=3)
    mats = torch.stack([aff.matrix(3, dtype, s) for s in (1.0, 0.5, -0.25)])
    mats[1, 0, 0] += 0.0625
    kw = dict(interpolation=2, bound="dct2", extrapolate=False)
    for m, a, w in ((moving[:1], mats, weight), (moving[:1], mats[:1], weight), (moving, mats, None)):
        want, allow = cpu.truth_and_allowance(m, fixed, a, w, TOL[dtype], 5, 1.0, **kw)
        got = interpol.lcc_gauss_newton_affine(dev(m), dev(fixed), dev(a), dev(w), window=5, eps=1.0, **kw)
        assert got[0].shape == (3,) and got[2].shape == (3, 12, 12)
        check(got, want, allow, "B=3 %s moving %d mat %d weight %s" % (dtype, m.shape[0], a.shape[0], w is not None))
    assert calls["n"] == 3


# ---------------------------------------------------------------------------------------------------------------------
# 2. routing
# ---------------------------------------------------------------------------------------------------------------------
def test_default_routing_reaches_the_fused_kernels_once(monkeypatch):
    calls = fused_calls(monkeypatch)
    assert isinstance(backend.fused_lcc_affine_orders, tuple) and set(backend.fused_lcc_affine_orders) <= set(ALL_ORDERS)
    for (inshape, shape), dtype in ((((7, 5, 6), (5, 6, 7)), F32), (((40, 64), (9, 33)), F64), (((200,), (257,)), F32)):
        dim = len(shape)
        moving, fixed, weight = (dev(t) for t in images(inshape, shape, 2200, dtype, B=2))
        mat = dev(aff.matrix(dim, dtype))
        for order in ALL_ORDERS:
            routed = order in backend.fused_lcc_affine_orders
            assert ops.lcc_affine_covered(moving, fixed, mat[None], weight, [order], [5] * dim) == routed
            before = calls["n"]
            loss, g, h = interpol.lcc_gauss_newton_affine(moving, fixed, mat, weight, window=5, interpolation=order)
            assert calls["n"] - before == routed
            assert loss.shape == (2,) and g.shape == (2, dim, dim + 1) and h.shape == (2, dim * (dim + 1), dim * (dim + 1))
            assert all(t.dtype == dtype and t.is_cuda for t in (loss, g, h))


@pytest.mark.parametrize("what", ["bf16", "4d", "mixed_orders", "window_11", "switched_off"])
def test_uncovered_classes_take_the_composed_route(what, monkeypatch):
    """Each case differs from a call that reaches the fused kernels in ONE property; the control is asserted to reach the binding."""
    route_all(monkeypatch)
    calls = fused_calls(monkeypatch)
    control = [dev(t) for t in images((7, 5, 6), (5, 6, 7), 2300, F32)]
    cmat = dev(aff.matrix(3, F32, 0.25))
    interpol.lcc_gauss_newton_affine(control[0], control[1], cmat, control[2], window=3, eps=1.0, interpolation=1)
    assert calls["n"] == 1
    order = [1, 2, 3] if what == "mixed_orders" else 1
    window = 11 if what == "window_11" else 3
    if what == "4d":
        gen = torch.Generator().manual_seed(5)
        moving, fixed, weight = torch.randn(2, 3, 4, 3, 4, generator=gen), torch.randn(2, 3, 3, 4, 3, generator=gen), None
        mat = torch.eye(5)[:4] + 0.0625 * torch.randn(4, 5, generator=gen).round()
    else:
        moving, fixed, weight = images((7, 5, 6), (5, 6, 7), 2300, torch.bfloat16 if what == "bf16" else F32)
        mat = aff.matrix(3, moving.dtype, 0.25)
    if what == "switched_off":
        monkeypatch.setattr(backend, "fused_lcc_affine_orders", ())
    kw = dict(interpolation=order, bound="dct2", extrapolate=True, window=window, eps=1.0)
    got = interpol.lcc_gauss_newton_affine(dev(moving), dev(fixed), dev(mat), dev(weight), **kw)
    assert calls["n"] == 1 and all(t.dtype == moving.dtype and t.is_cuda for t in got)
    want = interpol.lcc_gauss_newton_affine(moving.double(), fixed.double(), mat.double(), None if weight is None else weight.double(), **kw)
    tol = 2e-2 if what == "bf16" else 1e-4                                 # relative to the largest entry: the composed route in float32
    for g, w in zip(got, want):
        assert float((g.double().cpu() - w).abs().max()) <= tol * float(w.abs().max()), what


# ---------------------------------------------------------------------------------------------------------------------
# 3. bits
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_bits_do_not_depend_on_the_run_or_on_the_batch(dtype, monkeypatch):
    route_all(monkeypatch)
    for inshape, shape, order, hessian, window in (((7, 5, 6), (5, 6, 7), 3, True, 3), ((30, 8, 35), (33, 9, 33), 1, True, 9),
                                                   ((40, 64), (9, 33), 2, False, 5), ((200,), (257,), 2, True, 9)):
        dim = len(shape)
        moving, fixed, weight = (dev(t) for t in images(inshape, shape, 2400, dtype, B=3))
        mats = dev(torch.stack([aff.matrix(dim, dtype, s) for s in (1.0, 0.5, -0.25)]))
        kw = dict(interpolation=order, bound="dct2", extrapolate=False, hessian=hessian, window=window, eps=1.0)
        a = interpol.lcc_gauss_newton_affine(moving, fixed, mats, weight, **kw)
        b = interpol.lcc_gauss_newton_affine(moving, fixed, mats, weight, **kw)
        assert same(a, b), (shape, order)
        assert all(bool(t.isfinite().all()) for t in a if t is not None)
        if hessian:
            assert torch.equal(a[2], a[2].mT)
        for i in (0, 2):
            one = interpol.lcc_gauss_newton_affine(moving[i], fixed[0], mats[i], weight[i], **kw)
            assert same(one, [None if t is None else t[i] for t in a]), (shape, order, i)


def test_graph_replay_gives_the_bits_of_eager(monkeypatch):
    route_all(monkeypatch)
    moving, fixed, weight = (dev(t) for t in images((30, 8, 35), (33, 9, 33), 2500, F32, B=2))
    mat = dev(torch.stack([aff.matrix(3, F32), aff.matrix(3, F32, 0.5)]))
    kw = dict(interpolation=3, bound="dct2", extrapolate=True, window=5, eps=1.0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                        # warm-up on the side stream (module loads)
        interpol.lcc_gauss_newton_affine(moving, fixed, mat, weight, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = interpol.lcc_gauss_newton_affine(moving, fixed, mat, weight, **kw)
    for it in range(3):
        mat[:, :, -1] += 0.5 * (it + 1)
        graph.replay()
        torch.cuda.synchronize()
        eager = interpol.lcc_gauss_newton_affine(moving, fixed, mat, weight, **kw)
        assert same(out, eager), it
        assert bool(out[0].isfinite().all()) and bool((out[0] < 0).all()) and torch.equal(out[2], out[2].mT)


# ---------------------------------------------------------------------------------------------------------------------
# 4. memory contract
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("misalign", [0, 1, 3])
def test_memory_contract(misalign, dtype):
    for inshape, shape, hessian, window in (((7, 5, 6), (5, 6, 7), True, 3), ((30, 8, 35), (33, 9, 33), True, 9),
                                            ((40, 64), (9, 33), False, 5), ((200,), (257,), True, 9)):
        dim = len(shape)
        moving, fixed, weight = images(inshape, shape, 2600, dtype, B=2)
        mat = torch.stack([aff.matrix(dim, dtype), aff.matrix(dim, dtype, 0.5)])
        args = [moving, fixed, mat, weight]
        for bound, extrapolate in ((3, 1), (6, 0)):
            opt = ([bound] * 3, [3] * 3, extrapolate, hessian, [window] * dim, 1.0)
            ref = _hip.lcc_affine(*[dev(t) for t in args], *opt)
            assert all(bool(torch.isfinite(r).all()) for r in ref if r is not None)
            with memguard.installed(_hip, misalign=misalign) as seam:
                placed = [memguard.place(t, DEV, misalign=misalign) for t in args]
                out = _hip.lcc_affine(*placed, *opt)
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
# 5. more items than a launch has rows of workgroups
# ---------------------------------------------------------------------------------------------------------------------
# (name, dim, dtype, order, bound, extrapolate, hessian, eps): eps = 1 in float32 and 1e-5 in float64, for the reason tests/batch_loops.py gives
BATCH = [
    ("3d-f32-o2-dft-ex1", 3, F32, 2, "dft", True, True, 1.0),
    ("3d-f64-o1-dct2-ex1-nohess", 3, F64, 1, "dct2", True, False, 1e-5),
    ("1d-f32-o3-dct2-ex0", 1, F32, 3, "dct2", False, True, 1.0),
    ("1d-f64-o2-zero-ex0", 1, F64, 2, "zero", False, True, 1e-5),
]


def batch_matrices(dim, dtype, B):
    """one dyadic matrix per item: `matrix` (3-D: at a quarter of its translation) plus multiples of 1 / 32 in [-1/8, 1/8]"""
    gen = torch.Generator().manual_seed(BL.SEED + dim)
    return (aff.matrix(dim, F64, 0.25 if dim == 3 else 1.0)[None] + torch.randint(-4, 5, [B, dim, dim + 1], generator=gen).double() / 32).to(dtype)


@pytest.mark.parametrize("case", BATCH, ids=[c[0] for c in BATCH])
def test_more_items_than_rows_of_workgroups(case, monkeypatch):
    name, dim, dtype, order, bound, extrapolate, hessian, eps = case
    route_all(monkeypatch)
    calls = fused_calls(monkeypatch)
    B = BL.B_LOOP
    inshape, shape = BL.LCC_LATTICES[dim]
    moving, fixed, _, weight = BL.lcc_problem(dim, dtype, order, 2.0, B)
    fixed = fixed[None]
    mats = batch_matrices(dim, dtype, B)
    assert moving.shape[0] == B == 65538 and mats.shape[0] == B and weight.shape[0] == B
    if not extrapolate:
        inside = in_view(mats, inshape, shape)
        assert 0.40 <= inside < 1.0, inside
    kw = dict(interpolation=order, bound=bound, extrapolate=extrapolate)
    want, allow = cpu.truth_and_allowance(moving, fixed, mats, weight, TOL[dtype], 3, eps, **kw)
    fn = lambda m, a, w: interpol.lcc_gauss_newton_affine(m, dev(fixed), a, w, window=3, eps=eps, hessian=hessian, **kw)
    args = [dev(moving), dev(mats), dev(weight)]
    got = fn(*args)
    assert calls["n"] == 1 and got[0].shape == (B,) and got[1].shape == (B, dim, dim + 1)
    check(got, want, allow, "batch " + name, hessian)
    # the second trip of rows 0 .. 2 holds other numbers than the first
    assert all(abs(float(want[0][b]) - float(want[0][b - BL.ROWS])) > 1e-3 * abs(float(want[0][b])) for b in BL.SECOND_TRIP)
    assert same(got, BL.chunks(fn, args)) and calls["n"] == 4


# ---------------------------------------------------------------------------------------------------------------------
# 6. one Gauss-Newton step on the device as one captured graph
# ---------------------------------------------------------------------------------------------------------------------
def solve_spd(H, g):
    """H x = g by Gaussian elimination without pivoting (H symmetric positive definite), element-wise operations only: nothing
    that a graph capture cannot hold"""
    n = H.shape[-1]
    A = torch.cat([H, g.reshape(n, 1)], 1)
    for k in range(n):
        row = A[k] / A[k, k]
        A = A - A[:, k:k + 1] * row[None]
        A[k] = row
    return A[:, n]


def test_one_gauss_newton_step_as_one_graph_lowers_the_loss(monkeypatch):
    route_all(monkeypatch)
    calls = fused_calls(monkeypatch)
    moving, fixed = lcc.rescaled_blobs(24, 3, F64, DEV)
    mat = torch.eye(4, dtype=F64, device=DEV)[:3].clone()
    kw = dict(interpolation=3, bound="dct2", extrapolate=True, window=9, eps=1e-5)

    def step(a):
        loss, g, H = interpol.lcc_gauss_newton_affine(moving, fixed, a, **kw)
        H = H + 1e-9 * torch.diagonal(H).sum() * torch.eye(12, dtype=F64, device=DEV)
        return loss, a - solve_spd(H, g.reshape(-1)).reshape(3, 4)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(mat)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        before, new = step(mat)
    graph.replay()
    torch.cuda.synchronize()
    after = interpol.lcc_gauss_newton_affine(moving, fixed, new, hessian=False, **kw)[0]
    print("LCCAFFINE one step: loss %.6g -> %.6g" % (float(before), float(after)))
    assert calls["n"] == 3 and bool(new.isfinite().all())
    assert float(after) < float(before) < 0


# ---------------------------------------------------------------------------------------------------------------------
# 7. the entry points validate before launching
# ---------------------------------------------------------------------------------------------------------------------
def test_entry_points_validate_before_launching():
    L = _hip.lib()
    inshape, shape = (6, 5, 4), (5, 4, 7)
    N = 5 * 4 * 7
    moving, fixed, weight = (dev(t) for t in aff.problem(inshape, shape, 2800, F32, C=3, B=2))
    mat = dev(torch.stack([aff.matrix(3, F32), aff.matrix(3, F32, 0.5)]))
    sentinel = 4321.0
    loss = torch.full([2], sentinel, device=DEV)
    grad = torch.full([2, 3, 4], sentinel, device=DEV)
    hess = torch.full([2, 12, 12], sentinel, device=DEV)

    def problem(dim=3, order=(3, 3, 3), B=2, C=3, flags=_hip.FLAG_AFFINE_GRID):
        m = [moving.stride(0), moving.stride(1), *moving.stride()[2:]]
        f = [fixed.stride(0), fixed.stride(1), *fixed.stride()[2:], 0, 0]
        return _hip.make_problem(dim, F32, F32, [3] * 3, list(order), 1, B, C, inshape, shape, m, [0] * 5, f, flags)

    need = L.interpol_lcc_affine_workspace(ctypes.byref(problem()))
    # one slot per workgroup and item, a, c, f, the 73 x 1024 sums, then I and (dI, C) of the dtype
    assert need == 2 * 1 * 8 + 3 * 2 * 3 * N * 8 + 2 * 73 * 1024 * 8 + 2 * 3 * N * 4 + 2 * 2 * 3 * N * 4
    assert L.interpol_lcc_affine_workspace(ctypes.byref(problem(B=65536))) > 0          # the batch is walked in a loop
    assert L.interpol_lcc_affine_workspace(ctypes.byref(problem(dim=4))) == -1
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)

    def call(p, m=moving, f=fixed, a=mat, w=weight, lo=loss, g=grad, h=hess, wh=1, win=(3, 5, 3), eps=1.0, mbs=12, wbs=N, work=ws,
             nbytes=None):
        window = None if win is None else (ctypes.c_int * 3)(*win)
        return L.interpol_lcc_affine(ctypes.byref(p), ptr(m), ptr(f), ptr(a), ptr(w), ptr(lo), ptr(g), ptr(h), wh, window, eps, mbs, wbs,
                                     ptr(work), (0 if work is None else work.numel()) if nbytes is None else nbytes, ctypes.c_void_p(0))

    assert call(problem(dim=4)) == -1 and call(problem(order=(1, 2, 3))) == -2 and call(problem(C=0)) == -5 and call(problem(B=0)) == -5
    assert call(problem(flags=_hip.FLAG_DISPLACEMENT)) == -10
    for missing in ("m", "f", "a", "lo", "g", "h"):
        assert call(problem(), **{missing: None}) == -6                 # INTERPOL_E_NULL
    assert call(problem(), work=None, nbytes=need) == -6 and call(problem(), win=None) == -6
    assert call(problem(), nbytes=need - 1) == -9                       # INTERPOL_E_SCRATCH: a short workspace
    assert call(problem(), g=mat) == -10                                # the gradient is the matrix
    assert call(problem(), g=moving.view(-1)[7:]) == -10                # ... starts inside the moving image
    assert call(problem(), h=fixed) == -10 and call(problem(), lo=weight) == -10
    assert call(problem(), h=grad.view(-1)) == -10                      # two outputs that overlap
    assert call(problem(), work=hess.view(torch.uint8), nbytes=need) == -10           # the workspace is an output
    assert call(problem(), work=moving.view(torch.uint8), nbytes=need) == -10         # ... an input
    big = torch.zeros(need + 8, dtype=torch.uint8, device=DEV)
    assert call(problem(), work=big[4:], nbytes=need) == -10            # a workspace that is not 8-byte aligned
    huge = torch.zeros(2 * need, dtype=torch.uint8, device=DEV)
    assert call(problem(), work=huge, lo=huge[need - 8:].view(torch.float32), nbytes=need) == -10   # the loss inside the workspace
    for win in ((4, 5, 3), (3, 0, 3), (3, 5, 11), (3, 5, -1)):
        assert call(problem(), win=win) == -5                           # an even window, 0, above 9
    for eps in (0.0, -1.0, float("nan"), float("inf")):
        assert call(problem(), eps=eps) == -5
    for wh in (-1, 2):
        assert call(problem(), wh=wh) == -5
    assert call(problem(), mbs=-1) == -10 and call(problem(), wbs=-1) == -10
    torch.cuda.synchronize()
    assert all(bool((t == sentinel).all()) for t in (loss, grad, hess)) and not bool(ws.any())
    # valid calls: as the binding makes them; a NULL weight and a NULL Hessian with no Hessian asked for
    ref = _hip.lcc_affine(moving, fixed, mat, weight, [3] * 3, [3] * 3, 1, True, [3, 5, 3], 1.0)
    assert call(problem()) == 0
    torch.cuda.synchronize()
    assert torch.equal(loss, ref[0]) and torch.equal(grad, ref[1]) and torch.equal(hess, ref[2]) and bool(ws.any())
    hess.fill_(sentinel)
    assert call(problem(), w=None, h=None, wh=0, wbs=-1) == 0
    torch.cuda.synchronize()
    assert torch.equal(grad, _hip.lcc_affine(moving, fixed, mat, None, [3] * 3, [3] * 3, 1, False, [3, 5, 3], 1.0)[1])
    assert bool((hess == sentinel).all())
