"""`interpol.regulariser_solve` on the device (csrc/regulariser_solve.hip).

Truth: tests/test_regulariser_solve_cpu.py -- the algorithm restated in float64 on the dense spatial matrix of
tests/test_regulariser_cpu.py, and `torch.linalg.solve` of the assembled matrix -- on the inputs as the device sees them
(rounded to its dtype); never the code under test.

Bars.  Fixed iteration counts: |got - want| <= tol |want| + tol max|want|, tol = 1e-11 (float64) / 1e-5 (float32).  Converged:
1e-11 max|want| (float64), cond(A) 2^-23 max|want| (float32; cond from eigvalsh of the assembled matrix).

Cases of the fixed-count test: `cases_for` of the CPU module, where the reasoning is (no singular system, cond(A) bounded a
priori).  Three (shape, case) pairs are not compared at 24 iterations in float32, one of them not in float64 either
(FLOAT32_UNSTABLE_AT_24 / FLOAT64_UNSTABLE_AT_24: the reference's own float32 run, resp. its float64 run on a right-hand side
moved by one ulp, leaves the bar there, asserted by the CPU module), and bending alone on a shape with an extent of 1 or 2
runs in float64 only (`float32_floor_above_the_bar`: the rounding of the cancelling taps over the smallest eigenvalue).

Shapes: the smallest that can still break the kernels, for the reasons in the header of tests/test_regulariser_gpu.py: (130,)
and (19, 11) end inside a workgroup; (9, 5, 67) is twelve workgroups with a ragged last one that straddle rows and planes;
(5, 4, 23) is two; at (3, 3, 3), (1, 2, 3), (2, 1, 1) and (4, 2, 5) the 2-ring wraps more than once and almost all of the 1024
persistent workgroups of an item have no point.  Every solve is at most 200 iterations of five tiny launches.
"""
import ctypes

import pytest
import torch

import interpol
from interpol import _hip, backend, ops
import memguard
import test_regulariser_cpu as truth
import test_regulariser_solve_cpu as st

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = {torch.float32: 1e-5, torch.float64: 1e-11}
SHAPES = [(130,), (19, 11), (9, 5, 67), (5, 4, 23), (3, 3, 3), (1, 2, 3), (2, 1, 1), (4, 2, 5)]
IDS = ["x".join(map(str, s)) for s in SHAPES]
VOXELS = truth.VOXELS
field = truth.field


def fused_calls(monkeypatch):
    """count the calls that reach the entry point of the library"""
    calls = dict(solve=0)
    fn = _hip.regulariser_solve

    def f(*a, **k):
        calls["solve"] += 1
        return fn(*a, **k)

    monkeypatch.setattr(_hip, "regulariser_solve", f)
    return calls


def dev(t):
    return None if t is None else t.to(DEV)


# ---------------------------------------------------------------------------------------------------------------------
# 1. routing
# ---------------------------------------------------------------------------------------------------------------------
def test_default_routing_is_the_fused_kernels(monkeypatch):
    assert backend.fused_regulariser_solve is True
    calls = fused_calls(monkeypatch)
    for shape in ((130,), (19, 11), (9, 5, 67)):
        for dtype in (torch.float32, torch.float64):
            for kind in ("none", "diag", "full"):
                g = field(shape, 1, dtype).to(DEV)
                h = dev(st.hessian_arg(shape, 2, kind, dtype)[0])
                assert ops.regulariser_solve_covered(g, h)
                before = calls["solve"]
                x = interpol.regulariser_solve(g, h, absolute=0.1, membrane=1., max_iter=3)
                assert calls["solve"] - before == 1 and x.shape == g.shape and x.dtype == dtype and x.is_cuda


@pytest.mark.parametrize("what", ["bf16", "4d", "switched_off"])
def test_uncovered_classes_take_the_composed_route(what, monkeypatch):
    shape = (3, 2, 4, 3) if what == "4d" else (5, 4, 23)
    kw = dict(absolute=0.1, membrane=0.7, bending=0.3, bound="dct2", max_iter=8)
    g32 = field(shape, 7, torch.float32)
    h32 = st.hessian_arg(shape, 8, "full", torch.float32)[0]
    if what == "bf16":
        g, h = g32.bfloat16(), h32.bfloat16()
        g32, h32 = g.float(), h.float()
    else:
        g, h = g32, h32
    fused = None
    if what != "4d":
        fused = interpol.regulariser_solve(g32.to(DEV), h32.to(DEV), **kw)
    if what == "switched_off":
        monkeypatch.setattr(backend, "fused_regulariser_solve", False)
    calls = fused_calls(monkeypatch)
    assert not ops.regulariser_solve_covered(g.to(DEV), h.to(DEV))
    got, info = interpol.regulariser_solve(g.to(DEV), h.to(DEV), return_info=True, **kw)
    assert calls["solve"] == 0 and got.dtype == g.dtype and got.is_cuda and info.iterations.is_cuda
    assert info.iterations.tolist() == [8, 8]
    if what == "4d":
        # no fused kernel in 4-D: the composed form on the device against the composed form on the host, float32 bar
        want = interpol.regulariser_solve(g32.double(), h32.double(), **kw)
        assert st.close(got, want, TOL[torch.float32]) <= 1.0
    elif what == "bf16":
        assert float((got.float() - fused).abs().max()) <= 1e-2 * float(fused.abs().max())
    else:
        assert st.close(got, fused.cpu().double(), TOL[torch.float32]) <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# 2. fixed iteration counts against the restated algorithm
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(SHAPES)), ids=IDS)
def test_fixed_iteration_counts_match_the_restated_algorithm(case, monkeypatch):
    shape = SHAPES[case]
    dim = len(shape)
    calls = fused_calls(monkeypatch)
    worst = {torch.float32: 0.0, torch.float64: 0.0}
    n_calls = 0
    for n, (w, bound, vx, kind) in enumerate(st.cases_for(dim)):
        for dtype in (torch.float64, torch.float32):
            if dtype == torch.float32 and st.float32_floor_above_the_bar(shape, n):
                continue
            sy = st.system(shape, 100 * case + n, bound, w, vx, kind, dtype)
            want = st.want_after(("gpu", shape, n, dtype), sy, (1, 8, 24))
            g, h = dev(sy["g"]), dev(sy["h"])
            unstable = (shape, n) in (st.FLOAT32_UNSTABLE_AT_24 if dtype == torch.float32 else st.FLOAT64_UNSTABLE_AT_24)
            for k in ((1, 8) if unstable else (1, 8, 24)):
                for B in ((2, 1) if k == 8 else (2,)):
                    got, info = interpol.regulariser_solve(g[:B], None if h is None else h[:B], max_iter=k, tolerance=0.,
                                                           return_info=True, **sy["kw"])
                    n_calls += 1
                    assert got.dtype == dtype and info.iterations.shape == (B,) and bool((info.iterations <= k).all())
                    ratio = st.close(got, want[k][:B], TOL[dtype])
                    worst[dtype] = max(worst[dtype], ratio)
                    assert ratio <= 1.0, (shape, w, bound, vx, kind, dtype, k, B, ratio)
    assert calls["solve"] == n_calls
    print("fixed counts %s: worst error / bar: float32 %.3g, float64 %.3g" % (shape, worst[torch.float32], worst[torch.float64]))


# ---------------------------------------------------------------------------------------------------------------------
# 3. converged against the dense solve
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", range(len(st.CONVERGED)), ids=st.CONVERGED_IDS)
def test_converged_solution_is_the_dense_solve(case, dtype, monkeypatch):
    sy, want, cond = st.converged_truth(case, dtype)
    calls = fused_calls(monkeypatch)
    got, info = interpol.regulariser_solve(dev(sy["g"]), dev(sy["h"]), max_iter=200, return_info=True, **sy["kw"])
    assert calls["solve"] == 1 and got.dtype == dtype
    got = got.cpu().double()
    assert bool(torch.isfinite(got).all())
    for b in range(2):
        scale = float(want[b].abs().max())
        bar = TOL[dtype] * scale if dtype == torch.float64 else cond[b] * 2.0 ** -23 * scale
        err = float((got[b] - want[b]).abs().max())
        print("converged %s %s item %d: cond(A) = %.0f, error / bar = %.3g, iterations %d"
              % (st.CONVERGED[case][0], dtype, b, cond[b], err / bar, int(info.iterations[b])))
        assert err <= bar, (b, err / bar)


# ---------------------------------------------------------------------------------------------------------------------
# 4. determinism
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_bits_do_not_depend_on_the_run_or_on_the_batch(dtype):
    for shape, kind in (((9, 5, 67), "full"), ((19, 11), "diag"), ((130,), "none"), ((2, 1, 1), "full")):
        sy = st.system(shape, 40, "dct2", st.ALL, VOXELS[len(shape)], kind, dtype)
        g, h = dev(sy["g"]), dev(sy["h"])
        kw = dict(max_iter=12, tolerance=0., return_info=True, **sy["kw"])
        x, info = interpol.regulariser_solve(g, h, **kw)
        x2, info2 = interpol.regulariser_solve(g, h, **kw)
        assert torch.equal(x, x2) and torch.equal(info.iterations, info2.iterations) and torch.equal(info.residual, info2.residual)
        for b in range(2):
            xb, infob = interpol.regulariser_solve(g[b:b + 1], None if h is None else h[b:b + 1], **kw)
            assert torch.equal(xb[0], x[b]) and torch.equal(infob.residual[0], info.residual[b]), (shape, b)


def test_graph_replay_gives_the_bits_of_eager():
    shape = (9, 5, 67)
    kw = dict(absolute=0.3, membrane=0.7, bending=1.3, voxel_size=[2.0, 0.75, 1.5], bound="dct2", max_iter=10, tolerance=1e-2,
              return_info=True)
    gen = torch.Generator().manual_seed(9)
    g = torch.randn([2, *shape, 3], generator=gen).to(DEV)
    h = st.hessian_arg(shape, 41, "full", torch.float32)[0].to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                        # warm-up on the side stream (module loads)
        interpol.regulariser_solve(g, h, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        x, info = interpol.regulariser_solve(g, h, **kw)
    for it in range(3):
        g.copy_(torch.randn(g.shape, generator=gen) * (1 + it))
        graph.replay()
        torch.cuda.synchronize()
        xe, infoe = interpol.regulariser_solve(g, h, **kw)
        assert torch.equal(x, xe) and torch.equal(info.iterations, infoe.iterations) and torch.equal(info.residual, infoe.residual), it
        assert bool((info.iterations > 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# 5. stopping on the device
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_stopping(dtype, monkeypatch):
    calls = fused_calls(monkeypatch)
    st.check_stopping(DEV, dtype)
    assert calls["solve"] == 5


# ---------------------------------------------------------------------------------------------------------------------
# 6. memory contract
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("misalign", [0, 1, 3])
def test_memory_contract(misalign, dtype):
    weights = (0.3, 0.7, 1.3)
    for shape in ((9, 5, 67), (1, 2, 3), (19, 11), (130,), (2, 1, 1)):
        dim = len(shape)
        g = field(shape, 400 + dim, dtype)
        gd = g.to(DEV)
        for kind in ("none", "full"):
            h = st.hessian_arg(shape, 410 + dim, kind, dtype)[0]
            hd = dev(h)
            for bound in (3, 6):
                b, vx = [bound] * dim, VOXELS[dim]
                ref = _hip.regulariser_solve(gd, hd, weights, vx, b, 3, 0.)
                assert all(bool(torch.isfinite(r).all()) for r in ref)
                with memguard.installed(_hip, misalign=misalign) as seam:
                    gp = memguard.place(g, DEV, misalign=misalign)
                    hp = None if h is None else memguard.place(h, DEV, misalign=misalign)
                    out = _hip.regulariser_solve(gp, hp, weights, vx, b, 3, 0.)
                    torch.cuda.synchronize()
                    what = (shape, kind, bound, misalign)
                    assert len(seam.outputs()) == 2 and len(seam.workspaces()) == 1 and seam.workspace_was_written(), what
                    assert out[0].shape == g.shape and out[1].shape == (2, 2) and out[1].dtype == torch.float64, what
                    assert out[0].data_ptr() % memguard.ALIGN == misalign * g.element_size(), what
                    assert gp.data_ptr() % memguard.ALIGN == misalign * g.element_size(), what
                    for t, r in zip(out, ref):
                        seam.assert_fully_written(t, r, what)
                        assert torch.equal(t, r), what
                    seam.assert_guards_intact(what)
                    memguard.assert_guard_intact(gp, what)
                    assert torch.equal(gp, gd), what
                    if hp is not None:
                        memguard.assert_guard_intact(hp, what)
                        assert torch.equal(hp, hd), what


# ---------------------------------------------------------------------------------------------------------------------
# 7. views
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_views_with_an_offset_and_strided_fields(dim):
    shape = {1: (130,), 2: (19, 11), 3: (9, 5, 67)}[dim]
    g = field(shape, 500 + dim, torch.float32).to(DEV)
    h = st.hessian_arg(shape, 510 + dim, "full", torch.float32)[0].to(DEV)
    weights, vx, b = (0.3, 0.7, 1.3), VOXELS[dim], [3] * dim
    ref = _hip.regulariser_solve(g, h, weights, vx, b, 5, 0.)
    # a view whose storage starts one element into its buffer
    buf = torch.full([g.numel() + 1], float("nan"), device=DEV)
    view = buf[1:].view(g.shape)
    view.copy_(g)
    assert view.storage_offset() == 1 and view.data_ptr() % 8 != 0
    # a gradient stored channel-first (not point by point), and every other item of a larger batch
    chan = g.movedim(-1, 1).contiguous().movedim(1, -1)
    assert dim == 1 or not chan.is_contiguous()
    wide = torch.stack([g, g + 1], 1)[:, 0]
    assert wide.stride(0) == 2 * g.stride(0)
    # a Hessian that is not contiguous: the host makes it dense
    hchan = h.movedim(-1, 1).contiguous().movedim(1, -1)
    assert dim == 1 or not hchan.is_contiguous()
    for gv, hv in ((view, h), (chan, h), (wide, h), (g, hchan)):
        got = _hip.regulariser_solve(gv, hv, weights, vx, b, 5, 0.)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), dim
        x, info = interpol.regulariser_solve(gv, hv, 0.3, 0.7, 1.3, vx, "dct2", 5, 0., True)
        assert torch.equal(x, ref[0]) and torch.equal(info.residual, ref[1][:, 1]), dim
    # one Hessian for every item is not copied: batch stride 0
    one = _hip.regulariser_solve(g, h[:1], weights, vx, b, 5, 0.)
    assert torch.equal(one[0][0], ref[0][0])
    assert torch.equal(one[0], _hip.regulariser_solve(g, h[:1].expand_as(h).contiguous(), weights, vx, b, 5, 0.)[0])


# ---------------------------------------------------------------------------------------------------------------------
# 8. the entry points validate before launching
# ---------------------------------------------------------------------------------------------------------------------
def test_entry_points_validate_before_launching():
    L = _hip.lib()
    shp = (6, 5, 4)
    N = 6 * 5 * 4
    g = torch.randn(1, *shp, 3, device=DEV)
    H = st.hessian_arg(shp, 3, "full", torch.float32)[0][:1].contiguous().to(DEV)
    sentinel = 4321.0
    x = torch.full([1, *shp, 3], sentinel, device=DEV)
    info = torch.full([1, 2], sentinel, dtype=torch.float64, device=DEV)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    null = ctypes.c_void_p(0)
    vx = (ctypes.c_double * 3)(1., 1., 1.)

    def problem(dtype=torch.float32, dstr=None, C=3, dim=3, bound=3):
        s = [g.stride(0), 1, *g.stride()[1:4]]
        return _hip.make_problem(dim, dtype, dtype, [bound] * 3, [0] * 3, 1, 1, C, shp, shp, dstr or s, [0] * 5, [0] * 7, 0)

    need = L.interpol_regulariser_solve_workspace(ctypes.byref(problem()), 6)
    assert need >= 3 * N * 3 * 4 + 1024 * 2 * 8 + 8 * 8
    assert need == L.interpol_regulariser_solve_workspace(ctypes.byref(problem()), 0)    # a function of the problem alone
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)

    def solve(p, grad=g, hess=H, K=6, hbs=0, sol=x, w=(0., 1., 1.), h=vx, max_iter=2, tol=0., inf=info, work=ws, nbytes=None):
        return L.interpol_regulariser_solve(ctypes.byref(p), ptr(grad) if grad is not None else null, ptr(hess) if hess is not None else null,
                                            K, hbs, ptr(sol) if sol is not None else null, *w, h, max_iter, tol,
                                            ptr(inf) if inf is not None else null, ptr(work) if work is not None else null,
                                            work.numel() if nbytes is None else nbytes, null)

    assert solve(problem(dtype=torch.bfloat16)) == -4                   # INTERPOL_E_DTYPE
    assert solve(problem(dtype=torch.float16)) == -4
    assert L.interpol_regulariser_solve_workspace(ctypes.byref(problem(dtype=torch.bfloat16)), 6) == -4
    assert solve(problem(C=2)) == -5                                    # components != dims: INTERPOL_E_SHAPE
    assert solve(problem(), w=(0., -1., 1.)) == -5                      # a negative weight
    assert solve(problem(), w=(0., 0., 0.)) == -5                       # no term at all
    assert solve(problem(), h=(ctypes.c_double * 3)(1., 0., 1.)) == -5  # a voxel size that is not positive
    for K in (1, 2, 4, 5, 7, -1):
        assert solve(problem(), K=K) == -5                              # hessian_components
        assert L.interpol_regulariser_solve_workspace(ctypes.byref(problem()), K) == -5
    assert solve(problem(), max_iter=-1) == -5
    assert solve(problem(), tol=-1e-3) == -5
    for bound in (1, 2, 4, 7):
        assert solve(problem(bound=bound)) == -3                        # replicate, dct1, dst1, no bound at all: INTERPOL_E_BOUND
        assert L.interpol_regulariser_solve_workspace(ctypes.byref(problem(bound=bound)), 6) == -3
    assert solve(problem(dstr=[g.stride(0), 120, 20, 4, 1])) == -10     # a channel-first gradient: INTERPOL_E_STRIDE
    assert solve(problem(), hbs=-1) == -10
    assert solve(problem(), sol=g) == -10                               # the solution is the gradient
    assert solve(problem(), sol=g.view(-1)[7:]) == -10                  # ... starts inside it
    assert solve(problem(), sol=H) == -10                               # ... is the Hessian
    assert solve(problem(), work=H.view(torch.uint8).reshape(-1)[8:], nbytes=need) == -10     # the workspace inside the Hessian
    assert solve(problem(), work=g.view(torch.uint8), nbytes=need) == -10         # ... is the gradient
    assert solve(problem(), sol=ws.view(torch.float32)[64:]) == -10     # the solution inside the workspace
    assert solve(problem(), nbytes=need - 1) == -9                      # INTERPOL_E_SCRATCH
    assert solve(problem(), grad=None) == -6                            # INTERPOL_E_NULL
    assert solve(problem(), hess=None) == -6
    assert solve(problem(), sol=None) == -6
    assert solve(problem(), work=None, nbytes=need) == -6
    assert L.interpol_regulariser_solve(ctypes.byref(problem()), ptr(g), ptr(H), 6, 0, ptr(x), 0., 1., 1., None, 2, 0., ptr(info),
                                        ptr(ws), need, null) == -6     # no voxel sizes
    torch.cuda.synchronize()
    assert bool((x == sentinel).all()) and bool((info == sentinel).all()) and not bool(ws.any())
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(H).all())
    # a valid call; a NULL info and a NULL Hessian with no components are accepted
    assert solve(problem()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(x).all()) and not bool((x == sentinel).any()) and info.tolist()[0][0] == 2.0 and 0 < info.tolist()[0][1] < 1
    first = x.clone()
    x.fill_(sentinel)
    assert solve(problem(), inf=None) == 0
    torch.cuda.synchronize()
    assert torch.equal(x, first)
    assert solve(problem(), hess=None, K=0) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(x).all()) and not torch.equal(x, first)
