"""`interpol.regulariser_solve(preconditioner='multigrid')` on the device: the fused V-cycle and its conjugate gradients
(csrc/regulariser_multigrid.hip) against the float64 restatement of tests/test_multigrid_cpu.py (`mg`), which is never the code under
test: explicit level matrices from `interpol.regulariser` on identity fields, the prolongation as an explicit matrix.

Bars: |got - want| <= tol |want| + tol max|want| with tol 1e-11 (float64) / 1e-5 (float32), those of tests/test_regulariser_solve_gpu.py.
"""
import ctypes

import pytest
import torch

import interpol
from interpol import _hip, backend, ops
import memguard
import test_regulariser_cpu as truth
import test_regulariser_solve_cpu as st
import test_multigrid_cpu as mg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = {torch.float32: 1e-5, torch.float64: 1e-11}
DTYPES = [torch.float64, torch.float32]
CODES = dict(zero=0, dct2=3, dst2=5, dft=6, sliding=7)


def dev(t):
    return None if t is None else t.to(DEV)


def codes(bound, dim):
    return [CODES[b] for b in ([bound] * dim if isinstance(bound, str) else bound)]


def weights5(w):
    return tuple(float(w.get(k, 0.)) for k in mg.WEIGHT_NAMES)


def fused_calls(monkeypatch):
    """count the calls that reach the entry points of the library"""
    calls = dict(multigrid=0, cycle=0, jacobi=0)

    def counted(name, key):
        fn = getattr(_hip, name)

        def f(*a, **k):
            calls[key] += 1
            return fn(*a, **k)

        monkeypatch.setattr(_hip, name, f)

    counted("regulariser_multigrid_solve", "multigrid")
    counted("regulariser_multigrid_cycle", "cycle")
    counted("regulariser_solve", "jacobi")
    return calls


# ---------------------------------------------------------------------------------------------------------------------
# 5. one cycle against the dense V
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", mg.SHAPES, ids=mg.IDS)
def test_one_cycle_is_the_dense_cycle(shape, monkeypatch):
    calls = fused_calls(monkeypatch)
    dim = len(shape)
    worst, bad = {torch.float32: 0.0, torch.float64: 0.0}, []
    for n, (w, bound, vx, kind) in enumerate(mg.cases_for(shape)):
        for dtype in DTYPES:
            sy = mg.system(shape, 300 + n, bound, w, vx, kind, dtype)
            r = sy["g"].double()
            want = torch.stack([mg.vcycle(levels, r[b].reshape(-1, 1))[:, 0] for b, levels in enumerate(mg.levels_of((shape, n, dtype), sy))])
            got = ops.regulariser_vcycle(dev(sy["g"]), dev(sy["h"]) if sy["h"] is None or sy["h"].dim() == dim + 2 else dev(sy["h"][None]),
                                         weights5(w), st.voxels(dim, vx), codes(bound, dim))
            assert got.dtype == dtype and got.shape == sy["g"].shape
            ratio = st.close(got, want.reshape(r.shape), TOL[dtype])
            worst[dtype] = max(worst[dtype], ratio)
            if not ratio <= 1.0:
                bad.append((shape, w, bound, vx, kind, dtype, ratio))
    print("one cycle %s: worst error / bar: float32 %.3g, float64 %.3g" % (shape, worst[torch.float32], worst[torch.float64]))
    assert not bad, bad
    assert calls["cycle"] == 2 * len(mg.cases_for(shape))


# ---------------------------------------------------------------------------------------------------------------------
# 6. the fused solve at fixed iteration counts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", mg.SHAPES, ids=mg.IDS)
def test_fixed_iteration_counts_match_the_restated_algorithm(shape, monkeypatch):
    calls = fused_calls(monkeypatch)
    worst, bad = {torch.float32: 0.0, torch.float64: 0.0}, []
    n_calls = 0
    for n, (w, bound, vx, kind) in enumerate(mg.cases_for(shape)):
        for dtype in DTYPES:
            sy = mg.system(shape, 300 + n, bound, w, vx, kind, dtype)
            want = mg.want_after((shape, n, dtype), sy)
            for k in mg.ITERATIONS:
                got, info = interpol.regulariser_solve(dev(sy["g"]), dev(sy["h"]), max_iter=k, preconditioner="multigrid", return_info=True,
                                                       **sy["kw"])
                n_calls += 1
                assert got.dtype == dtype and info.iterations.shape == (2,) and bool((info.iterations <= k).all())
                ratio = st.close(got, want[k], TOL[dtype])
                print("fixed counts %s case %d %s k=%d: error / bar = %.3g" % (shape, n, dtype, k, ratio))
                worst[dtype] = max(worst[dtype], ratio)
                if not ratio <= 1.0:
                    bad.append((shape, w, bound, vx, kind, dtype, k, ratio))
    print("multigrid, fixed counts %s: worst error / bar: float32 %.3g, float64 %.3g" % (shape, worst[torch.float32], worst[torch.float64]))
    assert not bad, bad
    assert calls["multigrid"] == n_calls and calls["jacobi"] == 0


# ---------------------------------------------------------------------------------------------------------------------
# 7. converged: the dense solve, and info.residual recomputed
# ---------------------------------------------------------------------------------------------------------------------
# tiny definite systems: shape, bound, weights, voxel size
CONVERGED = [((16,), "dct2", dict(absolute=0.01, membrane=0.7, bending=1.3), 1.),
             ((16, 12), "dft", dict(bending=1.0), [0.5, 1.25]),
             ((8, 10), "sliding", dict(membrane=0.5, shears=1.0, div=2.0), 1.),
             ((5, 7), ["zero", "dst2"], dict(membrane=0.7, bending=0.3), 1.),
             ((8, 4, 10), ["zero", "dft", "dst2"], dict(membrane=0.7, bending=0.3), [2.0, 0.75, 1.5])]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("case", range(len(CONVERGED)), ids=["x".join(map(str, c[0])) for c in CONVERGED])
def test_converged_solution_is_the_dense_solve(case, dtype, monkeypatch):
    shape, bound, w, vx = CONVERGED[case]
    calls = fused_calls(monkeypatch)
    sy = mg.system(shape, 700 + case, bound, w, vx, "full", dtype)
    g, h = dev(sy["g"]), dev(sy["h"])
    got, info = interpol.regulariser_solve(g, h, max_iter=60, preconditioner="multigrid", return_info=True, **sy["kw"])
    assert calls["multigrid"] == 1 and got.dtype == dtype
    # the residual that `info` reports, recomputed with interpol.regulariser (float64)
    x64, g64 = got.double(), g.double()
    Hx = torch.einsum("bnde,bne->bnd", dev(sy["Hd"]), x64.reshape(2, -1, len(shape))).reshape(x64.shape)
    res = g64 - Hx - interpol.regulariser(x64, **sy["kw"])
    rel = res.reshape(2, -1).norm(dim=1) / g64.reshape(2, -1).norm(dim=1)
    for b, levels in enumerate(mg.levels_of(("converged", case, dtype), sy)):
        A = levels[0]["A"]
        assert float((A - A.t()).abs().max()) <= 1e-13 * float(A.abs().max())
        ev = torch.linalg.eigvalsh(0.5 * (A + A.t()))
        assert float(ev[0]) > 0
        cond = float(ev[-1] / ev[0])
        want = torch.linalg.solve(A, sy["g"][b].double().reshape(-1)).reshape(sy["g"][b].shape)
        scale = float(want.abs().max())
        bar = TOL[dtype] * scale if dtype == torch.float64 else cond * 2.0 ** -23 * scale
        err = float((got[b].cpu().double() - want).abs().max())
        print("multigrid converged %s %s item %d: cond(A) = %.0f, error / bar = %.3g, iterations %d, residual %.3g (recomputed %.3g)"
              % (shape, dtype, b, cond, err / bar, int(info.iterations[b]), float(info.residual[b]), float(rel[b])))
        assert err <= bar, (b, err / bar)
        # the recursively updated residual and the true one differ by the rounding of the run: cond eps relative to g
        eps = 2.0 ** -52 if dtype == torch.float64 else 2.0 ** -23
        assert abs(float(info.residual[b]) - float(rel[b])) <= 8 * cond * eps, (b, float(info.residual[b]), float(rel[b]))


def test_info_residual_is_the_recomputed_residual_before_convergence():
    shape, bound, w, vx = CONVERGED[1]
    sy = mg.system(shape, 701, bound, w, vx, "full")
    g, h = dev(sy["g"]), dev(sy["h"])
    x, info = interpol.regulariser_solve(g, h, max_iter=3, preconditioner="multigrid", return_info=True, **sy["kw"])
    Hx = torch.einsum("bnde,bne->bnd", dev(sy["Hd"]), x.reshape(2, -1, 2)).reshape(x.shape)
    res = g - Hx - interpol.regulariser(x, **sy["kw"])
    rel = res.reshape(2, -1).norm(dim=1) / g.reshape(2, -1).norm(dim=1)
    assert info.iterations.tolist() == [3, 3] and bool((info.residual > 1e-8).all())
    assert bool(((info.residual - rel).abs() <= 1e-11 * rel).all()), (info.residual, rel)


# ---------------------------------------------------------------------------------------------------------------------
# 8. the iteration count of the 64 x 64 case
# ---------------------------------------------------------------------------------------------------------------------
def test_iteration_count_of_the_prototype_system(monkeypatch):
    calls = fused_calls(monkeypatch)
    want, jac = mg.prototype_counts()
    g, h, _ = mg.prototype_system()
    x, info = interpol.regulariser_solve(dev(g), dev(h), bending=1.0, bound="dft", max_iter=100, tolerance=1e-6, preconditioner="multigrid",
                                         return_info=True)
    print("64 x 64 to 1e-6: fused multigrid %d iterations, restated %d, restated jacobi %d" % (int(info.iterations[0]), want, jac))
    assert calls["multigrid"] == 1 and abs(int(info.iterations[0]) - want) <= 1 and float(info.residual[0]) <= 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# 9. bits
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_bits_do_not_depend_on_the_run_or_on_the_batch(dtype):
    for shape, n in (((16, 8, 10), 2), ((16, 12), 0), ((16,), 2), ((5, 7), 5)):
        w, bound, vx, kind = mg.cases_for(shape)[n]
        sy = mg.system(shape, 40, bound, w, vx, kind, dtype)
        g, h = dev(sy["g"]), dev(sy["h"])
        kw = dict(max_iter=5, preconditioner="multigrid", return_info=True, **sy["kw"])
        x, info = interpol.regulariser_solve(g, h, **kw)
        x2, info2 = interpol.regulariser_solve(g, h, **kw)
        assert torch.equal(x, x2) and torch.equal(info.iterations, info2.iterations) and torch.equal(info.residual, info2.residual)
        for b in range(2):
            xb, infob = interpol.regulariser_solve(g[b:b + 1], None if h is None else h[b:b + 1], **kw)
            assert torch.equal(xb[0], x[b]) and torch.equal(infob.residual[0], info.residual[b]), (shape, b)


def test_graph_replay_gives_the_bits_of_eager():
    shape = (16, 8, 10)
    kw = dict(absolute=0.3, membrane=0.7, bending=1.3, voxel_size=[2.0, 0.75, 1.5], bound="dct2", max_iter=6, tolerance=1e-4,
              preconditioner="multigrid", return_info=True)
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


def test_a_done_item_keeps_its_bits():
    """an item that stops early is still cycled with the others; its x is that of a call that ends at its own count"""
    shape = (16, 12)
    w, bound, vx, kind = mg.cases_for(shape)[0]
    sy = mg.system(shape, 45, bound, w, vx, kind, torch.float32)
    g, h = dev(sy["g"]), dev(sy["h"])
    g[1] *= 1e3                                                          # (the relative residual is scale free; rounding is not)
    kw = dict(preconditioner="multigrid", return_info=True, **sy["kw"])
    x, info = interpol.regulariser_solve(g, h, max_iter=40, tolerance=1e-3, **kw)
    its = info.iterations.tolist()
    assert all(0 < i < 40 for i in its) and bool((info.residual <= 1e-3).all())
    for b in range(2):
        again, inf2 = interpol.regulariser_solve(g, h, max_iter=its[b], tolerance=0., **kw)
        assert torch.equal(again[b], x[b]) and float(inf2.residual[b]) == float(info.residual[b]), b
    g[0] = 0
    x0, info0 = interpol.regulariser_solve(g, h, max_iter=40, tolerance=1e-3, **kw)
    assert not bool(x0[0].any()) and int(info0.iterations[0]) == 0 and float(info0.residual[0]) == 0.0
    assert torch.equal(x0[1], x[1]) and bool(torch.isfinite(x0).all())


# ---------------------------------------------------------------------------------------------------------------------
# 10. memory contract
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("misalign", [0, 1, 3])
def test_memory_contract(misalign, dtype):
    weights = (0.3, 0.7, 1.3, 0., 0.)
    for shape in ((16, 8, 10), (5, 7), (16, 12), (16,)):
        dim = len(shape)
        g = truth.field(shape, 400 + dim, dtype)
        gd = g.to(DEV)
        for kind in ("none", "full"):
            h = st.hessian_arg(shape, 410 + dim, kind, dtype)[0]
            hd = dev(h)
            for bound in (3, 6):
                b, vx = [bound] * dim, truth.VOXELS[dim]
                for which in ("solve", "cycle"):
                    if which == "solve":
                        call = lambda gg, hh: _hip.regulariser_multigrid_solve(gg, hh, weights, vx, b, 2, 0., 2)
                    else:
                        call = lambda gg, hh: (_hip.regulariser_multigrid_cycle(gg, hh, weights, vx, b, 2),)
                    ref = call(gd, hd)
                    assert all(bool(torch.isfinite(r).all()) for r in ref)
                    with memguard.installed(_hip, misalign=misalign) as seam:
                        gp = memguard.place(g, DEV, misalign=misalign)
                        hp = None if h is None else memguard.place(h, DEV, misalign=misalign)
                        out = call(gp, hp)
                        torch.cuda.synchronize()
                        what = (shape, kind, bound, misalign, which)
                        assert len(seam.outputs()) == 2 and len(seam.workspaces()) == 1 and seam.workspace_was_written(), what
                        assert out[0].shape == g.shape and out[0].data_ptr() % memguard.ALIGN == misalign * g.element_size(), what
                        for t, r in zip(out, ref):
                            seam.assert_fully_written(t, r, what)
                            assert torch.equal(t, r), what
                        seam.assert_guards_intact(what)
                        memguard.assert_guard_intact(gp, what)
                        assert torch.equal(gp, gd), what
                        if hp is not None:
                            memguard.assert_guard_intact(hp, what)
                            assert torch.equal(hp, hd), what


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_views_with_an_offset_and_strided_fields(dim):
    shape = {1: (16,), 2: (16, 12), 3: (16, 8, 10)}[dim]
    g = truth.field(shape, 500 + dim, torch.float32).to(DEV)
    h = st.hessian_arg(shape, 510 + dim, "full", torch.float32)[0].to(DEV)
    weights, vx, b = (0.3, 0.7, 1.3, 0., 0.), truth.VOXELS[dim], [3] * dim
    ref = _hip.regulariser_multigrid_solve(g, h, weights, vx, b, 3, 0., 2)
    zref = _hip.regulariser_multigrid_cycle(g, h, weights, vx, b, 2)
    buf = torch.full([g.numel() + 1], float("nan"), device=DEV)
    view = buf[1:].view(g.shape)
    view.copy_(g)
    assert view.storage_offset() == 1 and view.data_ptr() % 8 != 0
    chan = g.movedim(-1, 1).contiguous().movedim(1, -1)
    wide = torch.stack([g, g + 1], 1)[:, 0]
    assert wide.stride(0) == 2 * g.stride(0)
    hchan = h.movedim(-1, 1).contiguous().movedim(1, -1)
    for gv, hv in ((view, h), (chan, h), (wide, h), (g, hchan)):
        got = _hip.regulariser_multigrid_solve(gv, hv, weights, vx, b, 3, 0., 2)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), dim
        assert torch.equal(_hip.regulariser_multigrid_cycle(gv, hv, weights, vx, b, 2), zref), dim
        x, info = interpol.regulariser_solve(gv, hv, 0.3, 0.7, 1.3, vx, "dct2", 3, 0., True, preconditioner="multigrid")
        assert torch.equal(x, ref[0]) and torch.equal(info.residual, ref[1][:, 1]), dim
    # one Hessian for every item is not copied (batch stride 0): the pyramid has one item as well
    one = _hip.regulariser_multigrid_solve(g, h[:1], weights, vx, b, 3, 0., 2)
    assert torch.equal(one[0][0], ref[0][0])
    assert torch.equal(one[0], _hip.regulariser_multigrid_solve(g, h[:1].expand_as(h).contiguous(), weights, vx, b, 3, 0., 2)[0])


def test_entry_points_validate_before_launching():
    L = _hip.lib()
    shp = (8, 6, 4)
    N = 8 * 6 * 4
    g = torch.randn(1, *shp, 3, device=DEV)
    H = st.hessian_arg(shp, 3, "full", torch.float32)[0][:1].contiguous().to(DEV)
    sentinel = 4321.0
    x = torch.full([1, *shp, 3], sentinel, device=DEV)
    info = torch.full([1, 2], sentinel, dtype=torch.float64, device=DEV)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    null = ctypes.c_void_p(0)
    vx = (ctypes.c_double * 3)(1., 1., 1.)
    w5 = lambda *w: (ctypes.c_double * 5)(*w)

    def problem(dtype=torch.float32, dstr=None, C=3, dim=3, bound=3):
        s = [g.stride(0), 1, *g.stride()[1:4]]
        return _hip.make_problem(dim, dtype, dtype, [bound] * 3, [0] * 3, 1, 1, C, shp, shp, dstr or s, [0] * 5, [0] * 7, 0)

    need = L.interpol_regulariser_multigrid_solve_workspace(ctypes.byref(problem()), 6)
    zneed = L.interpol_regulariser_multigrid_cycle_workspace(ctypes.byref(problem()), 6)
    # five fields, the slots and the scalars; one coarser level (4, 6, 4) with three fields and its Hessian
    assert need >= 5 * N * 3 * 4 + 1024 * 2 * 8 + 8 * 8 + (3 * 3 + 6) * (N // 2) * 4
    assert zneed >= N * 3 * 4 + (3 * 3 + 6) * (N // 2) * 4 and zneed < need
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)

    def solve(p, grad=g, hess=H, K=6, hbs=0, sol=x, w=w5(0., 1., 1., 0., 0.), h=vx, nu=2, max_iter=2, tol=0., inf=info, work=ws, nbytes=None):
        return L.interpol_regulariser_multigrid_solve(ctypes.byref(p), ptr(grad) if grad is not None else null,
                                                      ptr(hess) if hess is not None else null, K, hbs, ptr(sol) if sol is not None else null,
                                                      w, h, nu, max_iter, tol, ptr(inf) if inf is not None else null,
                                                      ptr(work) if work is not None else null, nbytes if nbytes is not None else (0 if work is None else work.numel()), null)

    def cycle(p, grad=g, hess=H, K=6, hbs=0, sol=x, w=w5(0., 1., 1., 0., 0.), h=vx, nu=2, work=ws, nbytes=None):
        return L.interpol_regulariser_multigrid_cycle(ctypes.byref(p), ptr(grad) if grad is not None else null,
                                                      ptr(hess) if hess is not None else null, K, hbs, ptr(sol) if sol is not None else null,
                                                      w, h, nu, ptr(work) if work is not None else null,
                                                      nbytes if nbytes is not None else (0 if work is None else work.numel()), null)

    for call in (solve, cycle):
        assert call(problem(dtype=torch.bfloat16)) == -4                # INTERPOL_E_DTYPE
        assert call(problem(C=2)) == -5                                 # components != dims: INTERPOL_E_SHAPE
        assert call(problem(), w=w5(0., -1., 1., 0., 0.)) == -5         # a negative weight
        assert call(problem(), w=w5(0., 0., 0., 0., 0.)) == -5          # no term at all
        assert call(problem(), h=(ctypes.c_double * 3)(1., 0., 1.)) == -5
        for K in (1, 2, 4, 5, 7, -1):
            assert call(problem(), K=K) == -5                           # hessian_components
        for nu in (0, -1):
            assert call(problem(), nu=nu) == -5                         # smoothing
        for bound in (1, 2, 4):
            assert call(problem(bound=bound)) == -3                     # replicate, dct1, dst1: INTERPOL_E_BOUND
        assert call(problem(), w=w5(0., 1., 0., 1., 0.)) == -3          # elastic weights under dct2
        assert call(problem(bound=7), w=w5(0., 1., 0., 1., 0.), nbytes=0) == -9    # ... sliding is taken (and the workspace is too small)
        assert call(problem(), hbs=-1) == -10                           # INTERPOL_E_STRIDE
        assert call(problem(dstr=[g.stride(0), 3, *g.stride()[1:4]])) == -10       # not point by point
        assert call(problem(), work=ws[1:], nbytes=need - 1) == -10     # a misaligned workspace
        assert call(problem(), sol=g) == -10                            # the output overlaps the input
        assert call(problem(), sol=H) == -10
        assert call(problem(), nbytes=(need if call is solve else zneed) - 1) == -9          # INTERPOL_E_SCRATCH
        assert call(problem(), grad=None) == -6 and call(problem(), sol=None) == -6 and call(problem(), work=None, nbytes=need) == -6
        assert call(problem(), hess=None) == -6 and call(problem(), hess=None, K=0) == 0
    assert L.interpol_regulariser_multigrid_solve_workspace(ctypes.byref(problem(dtype=torch.bfloat16)), 6) == -4
    assert L.interpol_regulariser_multigrid_cycle_workspace(ctypes.byref(problem()), 4) == -5
    assert solve(problem(), max_iter=-1) == -5 and solve(problem(), tol=-1e-3) == -5
    assert solve(problem(), inf=g) == -10
    torch.cuda.synchronize()
    # nothing was launched by a refused call: only the two accepted ones (K = 0) wrote x; refuse once more on fresh sentinels
    x.fill_(sentinel)
    info.fill_(sentinel)
    assert solve(problem(), K=4) == -5 and cycle(problem(), nu=0) == -5
    torch.cuda.synchronize()
    assert bool((x == sentinel).all()) and bool((info == sentinel).all())
    assert solve(problem()) == 0 and cycle(problem(), sol=torch.empty_like(x)) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(x).all()) and not bool((x == sentinel).any())


# ---------------------------------------------------------------------------------------------------------------------
# 11. routing
# ---------------------------------------------------------------------------------------------------------------------
def test_default_routing_is_the_fused_kernels(monkeypatch):
    assert backend.fused_regulariser_multigrid is True
    calls = fused_calls(monkeypatch)
    for shape in ((16,), (16, 12), (16, 8, 10)):
        for dtype in DTYPES:
            for kind in ("none", "diag", "full"):
                g = truth.field(shape, 1, dtype).to(DEV)
                h = dev(st.hessian_arg(shape, 2, kind, dtype)[0])
                assert ops.regulariser_multigrid_covered(g, h)
                before = dict(calls)
                x = interpol.regulariser_solve(g, h, absolute=0.1, membrane=1., max_iter=3, preconditioner="multigrid")
                assert calls["multigrid"] - before["multigrid"] == 1 and calls["jacobi"] == before["jacobi"]
                assert x.shape == g.shape and x.dtype == dtype and x.is_cuda
                y = interpol.regulariser_solve(g, h, absolute=0.1, membrane=1., max_iter=3, preconditioner="jacobi")
                assert calls["jacobi"] - before["jacobi"] == 1 and calls["multigrid"] - before["multigrid"] == 1
                assert torch.equal(y, interpol.regulariser_solve(g, h, absolute=0.1, membrane=1., max_iter=3))


@pytest.mark.parametrize("what", ["bf16", "4d", "switched_off"])
def test_uncovered_classes_take_the_composed_route(what, monkeypatch):
    shape = (8, 3, 2, 3) if what == "4d" else (16, 8, 10)
    kw = dict(absolute=0.1, membrane=0.7, bending=0.3, bound="dct2", max_iter=4, preconditioner="multigrid")
    g32 = truth.field(shape, 7, torch.float32)
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
        monkeypatch.setattr(backend, "fused_regulariser_multigrid", False)
    calls = fused_calls(monkeypatch)
    assert not ops.regulariser_multigrid_covered(g.to(DEV), h.to(DEV))
    got, info = interpol.regulariser_solve(g.to(DEV), h.to(DEV), return_info=True, **kw)
    assert calls["multigrid"] == 0 and got.dtype == g.dtype and got.is_cuda and info.iterations.is_cuda
    assert info.iterations.tolist() == [4, 4]
    if what == "4d":
        want = interpol.regulariser_solve(g32.double(), h32.double(), **kw)
        assert st.close(got, want, TOL[torch.float32]) <= 1.0
    elif what == "bf16":
        assert float((got.float() - fused).abs().max()) <= 1e-2 * float(fused.abs().max())
    else:
        assert st.close(got, fused.cpu().double(), TOL[torch.float32]) <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# 12. more items than a launch has rows of workgroups
# ---------------------------------------------------------------------------------------------------------------------
def batched_truth(g, H, w, k):
    """The restatement for B items of shape (n,), D = 1, at once: g, H (B, n) float64 -> x after k iterations (no item stops: the
    systems are definite).  The matrices are those of `mg` -- L_l from interpol.regulariser on identity fields, P explicit --
    with the per-item diagonal H added."""
    n = g.shape[1]
    (s0, hv), (s1, _) = mg.level_shapes((n,))
    w1 = {a: 2 * v for a, v in w.items()}
    L0, L1 = mg.dense_L(s0, w, [1.], "dct2"), mg.dense_L(s1, w1, [2.], "dct2")
    P = mg.dense_P(s0, hv, "dct2")
    H1 = 4 * (H[:, 0::2] + H[:, 1::2])
    A0, A1 = L0 + torch.diag_embed(H), L1 + torch.diag_embed(H1)
    M0, M1 = 1 / (H + mg.centre5(w, [1.])), 1 / (H1 + mg.centre5(w1, [2.]))
    mv = lambda A, v: torch.einsum("bij,bj->bi", A, v)

    def V(r):
        x = 0.5 * M0 * r
        x = x + 0.5 * M0 * (r - mv(A0, x))
        r1 = (r - mv(A0, x)) @ P
        e = 0.5 * M1 * r1
        for _ in range(mg.COARSEST_SWEEPS - 1):
            e = e + 0.5 * M1 * (r1 - mv(A1, e))
        x = x + e @ P.t()
        for _ in range(2):
            x = x + 0.5 * M0 * (r - mv(A0, x))
        return x

    x, r = torch.zeros_like(g), g.clone()
    z = V(r)
    p, rho = z.clone(), (r * z).sum(1)
    for _ in range(k):
        q = mv(A0, p)
        alpha = rho / (p * q).sum(1)
        x, r = x + alpha[:, None] * p, r - alpha[:, None] * q
        z = V(r)
        rho1 = (r * z).sum(1)
        p, rho = z + (rho1 / rho)[:, None] * p, rho1
    return x


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_more_items_than_rows_of_workgroups(dtype, monkeypatch):
    import batch_loops as BL
    calls = fused_calls(monkeypatch)
    B, n, k = BL.B_LOOP, 8, 2
    assert B == 65538 and len(mg.level_shapes((n,))) == 2
    w = dict(absolute=0.3, membrane=0.7, bending=1.3)
    gen = torch.Generator().manual_seed(12)
    g = torch.randn([B, n, 1], generator=gen, dtype=torch.float64).to(dtype)
    h = (0.2 * torch.rand([B, n, 1], generator=gen, dtype=torch.float64)).to(dtype)
    want = batched_truth(g.double()[..., 0], h.double()[..., 0], w, k)[..., None]
    # the batched restatement is the per-item one
    for b in BL.PINNED:
        levels = mg.build_levels((n,), "dct2", w, 1., h[b].double().reshape(n, 1, 1))
        one = mg.pcg(levels[0]["A"], mg.multigrid_prec(levels), g[b].double().reshape(-1), k)[0]
        assert float((one - want[b, :, 0]).abs().max()) <= 1e-13 * float(one.abs().max())
    kw = dict(bound="dct2", max_iter=k, preconditioner="multigrid", **w)

    def solve(a, c):
        x, info = interpol.regulariser_solve(a, c, return_info=True, **kw)
        return x, info.iterations, info.residual

    gd, hd = dev(g), dev(h)
    whole = solve(gd, hd)
    assert calls["multigrid"] == 1 and bool((whole[1] == k).all())
    ratio = st.close(whole[0], want, TOL[dtype])
    print("BATCH multigrid %s: B %d, error / bar = %.3g" % (dtype, B, ratio))
    assert ratio <= 1.0, ratio
    parts = BL.chunks(solve, [gd, hd], size=B // 2)                      # two slices, one trip of the batch loops each
    assert calls["multigrid"] == 3 and all(torch.equal(a, b) for a, b in zip(whole, parts))
