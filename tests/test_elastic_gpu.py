"""The linear-elastic terms (`shears`, `div`) and the 'sliding' bound of `interpol.regulariser` / `regulariser_energy` /
`regulariser_solve` on the device (csrc/regulariser_at.hpp: the mode bit M_EL of reg_at; the interpol_regulariser_elastic* entry points).

Truth: the float64 matrix of the full (N D x N D) operator of tests/test_elastic_cpu.py (`entries`, `apply_entries`,
`energy_entries`, `dense`), applied to the field as the device sees it (rounded to its dtype); for the solve at fixed iteration
counts the composed algorithm on the host in float64, which that module holds to the dense solve.  Never the code under test.

Bars: those of tests/test_regulariser_gpu.py and tests/test_regulariser_solve_gpu.py.  L v on randn fields:
|got - want| <= tol |want| + tol max|want|, tol = 1e-5 (float32) / 1e-11 (float64); the energy: rtol = tol with absolute > 0;
gradients: the L v bar against L^T g, resp. g 0.5 (L + L^T) v; smooth fields: n 2^-24 ||L||_inf max|v| (see the test); the solve
at fixed counts: the L v bar; converged: 1e-11 max|want| (float64), cond(A) 2^-23 max|want| (float32).

Shapes: those of tests/test_regulariser_gpu.py, for its reasons (ragged workgroups, rows and planes straddled, stencils wider
than the volume), and (6, 1, 7): an extent of 1 in a sliding dimension, where both neighbours of component 1 along dimension 1
are the point itself with the sign flipped.  B = 2 and B = 1.
"""
import ctypes

import pytest
import torch

import interpol
from interpol import _hip, backend, ops
import memguard
import test_elastic_cpu as el
import test_regulariser_solve_cpu as st

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = {torch.float32: 1e-5, torch.float64: 1e-11}
SHAPES = el.DEVICE_SHAPES                                                # (130,), (19, 11), (9, 5, 67), (3, 3, 3), (1, 2, 3), (2, 1, 1), (4, 2, 5), (6, 1, 7)
IDS = el.ids(SHAPES)
VOXELS = el.VOXELS
FIVE = el.FIVE
OLD = dict(absolute=0.3, membrane=0.7, bending=1.3)
MIX_A, MIX_B = ["sliding", "zero", "dft"], ["dft", "sliding", "sliding"]
# (weights, bound, anisotropic)
CASES = ([(dict(shears=0.6, div=0.9), "dft", False), (dict(shears=1.0), "dft", False), (dict(div=1.0), "dft", False),
          (dict(absolute=2.0, shears=0.6, div=0.9), "sliding", False), (dict(membrane=0.7, shears=0.6, div=0.9), "sliding", False),
          (dict(bending=1.3, shears=0.6, div=0.9), "sliding", False)]
         + [(FIVE, b, False) for b in el.NAMES]
         + [(FIVE, "sliding", False), (FIVE, MIX_A, False), (FIVE, MIX_B, False), (OLD, "sliding", False), (dict(membrane=1.0), MIX_B, False),
            (FIVE, "sliding", True), (FIVE, MIX_A, True)])
SYMMETRIC = ("zero", "dft", "sliding")                                   # with elastic weights

field = el.field
assert_close = el.assert_close


def per_dim(bound, dim):
    return bound if isinstance(bound, str) else bound[:dim]


def fused_calls(monkeypatch):
    """count the calls that reach the entry points of the library"""
    calls = dict(matvec=0, energy=0, solve=0)
    fns = dict(matvec=_hip.regulariser, energy=_hip.regulariser_energy, solve=_hip.regulariser_solve)

    def counted(name):
        def f(*a, **k):
            calls[name] += 1
            return fns[name](*a, **k)
        return f

    monkeypatch.setattr(_hip, "regulariser", counted("matvec"))
    monkeypatch.setattr(_hip, "regulariser_energy", counted("energy"))
    monkeypatch.setattr(_hip, "regulariser_solve", counted("solve"))
    return calls


# ---------------------------------------------------------------------------------------------------------------------
# 1. forward and energy against the dense matrix
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", range(len(SHAPES)), ids=IDS)
def test_forward_matches_the_dense_matrix(case, dtype, monkeypatch):
    shape = SHAPES[case]
    dim = len(shape)
    v = field(shape, 100 + case, dtype)
    vd = v.to(DEV)
    calls = fused_calls(monkeypatch)
    for w, bound, aniso in CASES:
        bound = per_dim(bound, dim)
        vx = VOXELS[dim] if aniso else 1.
        E = el.entries(shape, bound, vx, **w)
        want = el.apply_entries(E, v)
        assert float(want.abs().max()) > 0.1 * float(v.abs().max())        # (randn: the bar is not vacuous)
        for B in (2, 1):
            assert ops.regulariser_covered(vd[:B])
            got = interpol.regulariser(vd[:B], voxel_size=vx, bound=bound, **w)
            assert got.dtype == dtype
            assert_close(got, want[:B], TOL[dtype], (shape, w, bound, vx, B))
    assert calls["matvec"] == 2 * len(CASES) and calls["energy"] == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", range(len(SHAPES)), ids=IDS)
def test_energy_matches_the_dense_matrix(case, dtype, monkeypatch):
    shape = SHAPES[case]
    dim = len(shape)
    v = field(shape, 200 + case, dtype)
    vd = v.to(DEV)
    calls = fused_calls(monkeypatch)
    n = 0
    for w, bound, aniso in CASES:
        if not w.get("absolute"):
            w = dict(absolute=2.0, **w)                                   # (the energy well away from zero, as in the module of the three terms)
        bound = per_dim(bound, dim)
        vx = VOXELS[dim] if aniso else 1.
        E = el.entries(shape, bound, vx, **w)
        want = el.energy_entries(E, v)
        assert bool((want > 0.1 * v.double().square().reshape(2, -1).sum(1)).all()), (shape, w, bound)
        kw = dict(voxel_size=vx, bound=bound, **w)
        En = interpol.regulariser_energy(vd, **kw)
        assert En.shape == (2,) and En.dtype == dtype
        rel = (En.cpu().double() - want).abs() / want.abs()
        assert bool((rel <= TOL[dtype]).all()), (shape, w, bound, vx, float(rel.max()))
        # two identical calls give identical bits, and an item gives the same bits alone and inside the batch
        assert torch.equal(En, interpol.regulariser_energy(vd, **kw))
        assert torch.equal(En[:1], interpol.regulariser_energy(vd[:1], **kw))
        assert torch.equal(En[1:], interpol.regulariser_energy(vd[1:], **kw))
        n += 4
    assert calls["energy"] == n and calls["matvec"] == 0


def test_matvec_bits_do_not_depend_on_the_run_or_on_the_batch():
    for shape in ((9, 5, 67), (19, 11), (6, 1, 7)):
        dim = len(shape)
        vd = field(shape, 250, torch.float32).to(DEV)
        kw = dict(voxel_size=VOXELS[dim], bound="sliding", **FIVE)
        out = interpol.regulariser(vd, **kw)
        assert torch.equal(out, interpol.regulariser(vd, **kw))
        assert torch.equal(out[1:], interpol.regulariser(vd[1:], **kw))


# ---------------------------------------------------------------------------------------------------------------------
# 2. smooth fields: the a-priori bound
# ---------------------------------------------------------------------------------------------------------------------
def smooth_field(shape, B=2):
    """a few voxels of amplitude, one period (dft) per extent: max|L v| is small against ||L||_inf max|v|"""
    dim = len(shape)
    x = interpol.identity_grid(shape, dtype=torch.float64)
    phase = sum(2 * torch.pi * (x[..., d] + 0.5) / shape[d] for d in range(dim))
    comps = [3.0 * torch.sin(phase + 0.7 * c) + 1.5 * torch.cos(2 * torch.pi * (x[..., c] + 0.5) / shape[c]) for c in range(dim)]
    u = torch.stack(comps, -1)
    return torch.stack([u * (1 + 0.25 * b) for b in range(B)])


@pytest.mark.parametrize("shape", [(130,), (19, 11), (9, 5, 67)], ids=["1d", "2d", "3d"])
def test_smooth_field_precision(shape):
    """float32, |got - want| <= n 2^-24 ||L||_inf max|v| with n = 44: the 32 of tests/test_regulariser_gpu.py for the chain of
    reg_at behind one output in 3-D with absolute, membrane and bending, and 12 more for the elastic terms: the centre
    coefficient of a component swaps the common own-axis tap for the component's (2: one subtraction, one addition); each
    output takes 8 fused multiply-adds from the two other components on the diagonals (8; the +-1 factors of the taps are
    exact); the cross coefficient is rounded once from double and applied by one fused multiply-add onto the rounded product
    with h_d^2 (2).  ||L||_inf: the sum of the absolute taps of a row before folded taps are merged (the kernel does not merge
    them), from the entries of the truth."""
    n = 44
    dim = len(shape)
    v = smooth_field(shape).float()
    vd = v.to(DEV)
    worst = 0.0
    for w in (dict(shears=0.6, div=0.9), dict(membrane=0.7, shears=1.0), FIVE):
        for bound, vx in (("dft", 1.), ("sliding", 1.), ("dft", VOXELS[dim])):
            E = el.entries(shape, bound, vx, **w)
            want = el.apply_entries(E, v)
            bar = n * 2.0 ** -24 * el.norm_inf(E) * float(v.abs().max())
            got = interpol.regulariser(vd, voxel_size=vx, bound=bound, **w).cpu().double()
            ratio = float((got - want).abs().max()) / bar
            print("smooth %s %s %s vx=%s: error / bound = %.4f" % (shape, w, bound, vx, ratio))
            worst = max(worst, ratio)
            assert ratio <= 1.0, (shape, w, bound, vx, ratio)
    print("smooth %s: worst error / bound = %.4f" % (shape, worst))


# ---------------------------------------------------------------------------------------------------------------------
# 3. backward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", [(130,), (19, 11), (9, 5, 67), (1, 2, 3), (6, 1, 7)], ids=["1d", "2d", "3d", "tiny", "flat"])
def test_backward_is_the_transposed_matrix(shape, dtype, monkeypatch):
    dim = len(shape)
    v = field(shape, 300 + dim, dtype)
    g = field(shape, 310 + dim, dtype)
    ge = torch.tensor([0.7, -1.9], dtype=torch.float64).to(dtype)
    calls = fused_calls(monkeypatch)
    vx = VOXELS[dim]
    for bound in el.NAMES + ["sliding", MIX_A[:dim], MIX_B[:dim], ["sliding", "dct2", "dft"][:dim]]:
        symmetric = all(b in SYMMETRIC for b in ([bound] if isinstance(bound, str) else bound))
        E = el.entries(shape, bound, vx, **FIVE)
        kw = dict(voxel_size=vx, bound=bound, **FIVE)
        x = v.to(DEV).requires_grad_()
        before = dict(calls)
        got, = torch.autograd.grad(interpol.regulariser(x, **kw), x, g.to(DEV))
        # the forward always reaches the fused kernel; the backward does where L is symmetric and must not where it is not
        assert calls["matvec"] - before["matvec"] == (2 if symmetric else 1), bound
        assert_close(got, el.apply_entries(E, g, transpose=True), TOL[dtype], ("matvec", shape, bound))
        before = dict(calls)
        got, = torch.autograd.grad(interpol.regulariser_energy(x, **kw), x, ge.to(DEV))
        assert (calls["energy"] - before["energy"], calls["matvec"] - before["matvec"]) == (1, 1 if symmetric else 0), bound
        want = 0.5 * (el.apply_entries(E, v) + el.apply_entries(E, v, transpose=True)) * ge.double().reshape([2] + [1] * (dim + 1))
        assert_close(got, want, TOL[dtype], ("energy", shape, bound))
    # the three old terms keep their symmetric set, and gain sliding
    for bound, symmetric in (("dct2", True), ("dst2", True), ("sliding", True), ("replicate", False)):
        x = v.to(DEV).requires_grad_()
        before = dict(calls)
        torch.autograd.grad(interpol.regulariser(x, bound=bound, **OLD), x, g.to(DEV))
        assert calls["matvec"] - before["matvec"] == (2 if symmetric else 1), bound


def test_gradcheck_and_double_backward_on_the_device(monkeypatch):
    kw = dict(voxel_size=[2.0, 0.75, 1.5], bound="sliding", **FIVE)
    v = field((4, 3, 5), 33, B=1).to(DEV).requires_grad_()
    calls = fused_calls(monkeypatch)
    assert torch.autograd.gradcheck(lambda x: interpol.regulariser(x, **kw), (v,))
    assert torch.autograd.gradcheck(lambda x: interpol.regulariser_energy(x, **kw), (v,))
    assert calls["matvec"] > 0 and calls["energy"] > 0
    # L is linear: the second derivative of sum (L v)^2 is 2 L^T L, every application of L on the fused kernel
    E = el.entries((4, 3, 5), "sliding", [2.0, 0.75, 1.5], **FIVE)
    v = field((4, 3, 5), 34).to(DEV).requires_grad_()
    g1, = torch.autograd.grad(interpol.regulariser(v, **kw).square().sum(), v, create_graph=True)
    z = field((4, 3, 5), 35)
    g2, = torch.autograd.grad(g1, v, z.to(DEV))
    assert_close(g2, 2 * el.apply_entries(E, el.apply_entries(E, z), transpose=True), 1e-11, "double backward")


@pytest.mark.parametrize("what", ["bf16", "4d", "switched_off"])
def test_uncovered_classes_take_the_composed_route(what, monkeypatch):
    dtype = torch.bfloat16 if what == "bf16" else torch.float32
    shape = (3, 4, 2, 5) if what == "4d" else (9, 5, 67)
    dim = len(shape)
    if what == "switched_off":
        monkeypatch.setattr(backend, "fused_regulariser", False)
    v = field(shape, 7, dtype)
    vd = v.to(DEV)
    calls = fused_calls(monkeypatch)
    assert not ops.regulariser_covered(vd)
    w = dict(absolute=2.0, membrane=0.7, bending=0.3, shears=0.6, div=0.9)
    tol = 1e-2 if what == "bf16" else 1e-5
    E = el.entries(shape, "sliding", 1., **w)
    got = interpol.regulariser(vd, bound="sliding", **w)
    En = interpol.regulariser_energy(vd, bound="sliding", **w)
    assert calls == dict(matvec=0, energy=0, solve=0) and got.dtype == dtype and En.dtype == dtype
    assert_close(got.float(), el.apply_entries(E, v.float()), tol, what)
    want = el.energy_entries(E, v.float())
    assert bool(((En.cpu().double() - want).abs() <= tol * want.abs()).all()), what


# ---------------------------------------------------------------------------------------------------------------------
# 4. the solve
# ---------------------------------------------------------------------------------------------------------------------
solve_cases, host_runs, UNSTABLE = el.solve_cases, el.host_runs, el.UNSTABLE


@pytest.mark.parametrize("case", range(len(SHAPES)), ids=IDS)
def test_fixed_iteration_counts_match_the_composed_algorithm(case, monkeypatch):
    """float64 at the 1e-11 bar and float32 at the 1e-5 bar, after 1, 8 and 24 iterations, for every case of `solve_cases` but the
    eight named in `UNSTABLE` of tests/test_elastic_cpu.py, whose reason that module asserts on the host.  The number of runs
    compared is asserted.  The iteration count must be the reference's while its residual is above rounding; past that,
    when an item stops is rounding too."""
    shape = SHAPES[case]
    dim = len(shape)
    worst = {torch.float32: 0.0, torch.float64: 0.0}
    compared = {torch.float32: 0, torch.float64: 0}
    for n, (w, bound, vx, kind) in enumerate(solve_cases(dim)):
        g, h, kw = el.device_system(case, n)
        runs = host_runs((shape, n), g, h, kw, (1, 8, 24))
        calls = fused_calls(monkeypatch)
        for dtype in (torch.float64, torch.float32):
            gd, hd = g.to(DEV, dtype), None if h is None else h.to(DEV, dtype)
            for k in (1, 8, 24):
                want, its, res = runs[torch.float64, k]
                if (shape, n, dtype, k) in UNSTABLE:
                    continue
                for B in ((2, 1) if k == 8 else (2,)):
                    before = calls["solve"]
                    got, info = interpol.regulariser_solve(gd[:B], None if hd is None else hd[:B], max_iter=k, tolerance=0.,
                                                           return_info=True, **kw)
                    assert calls["solve"] == before + 1
                    assert got.dtype == dtype and info.iterations.shape == (B,) and info.residual.dtype == torch.float64
                    assert bool((info.iterations.cpu() <= k).all())
                    if bool((res[:B] > 1e3 * TOL[dtype]).all()):
                        assert info.iterations.cpu().tolist() == its[:B].tolist(), (shape, n, dtype, k)
                    ratio = st.close(got, want[:B], TOL[dtype])
                    worst[dtype] = max(worst[dtype], ratio)
                    compared[dtype] += 1
                    assert ratio <= 1.0, (shape, w, bound, vx, kind, dtype, k, B, ratio)
                    # the relative residual sqrt(sigma / gamma): to three digits less than the fields, and not below their
                    # precision (a converged residual is rounding alone)
                    rr = (info.residual.cpu() - res[:B]).abs() / (1e3 * TOL[dtype] * res[:B] + TOL[dtype])
                    assert bool((rr <= 1.0).all()), (shape, n, dtype, k, float(rr.max()))
    for dtype in compared:                                               # (1 and 24 iterations: B = 2; 8: B = 2 and B = 1)
        left_out = sum(2 if k == 8 else 1 for (sh, _, dt, k) in UNSTABLE if sh == shape and dt == dtype)
        assert compared[dtype] == 4 * len(solve_cases(dim)) - left_out, (shape, dtype, compared[dtype])
    print("fixed counts %s: worst error / bar: float32 %.3g (%d runs), float64 %.3g (%d runs)"
          % (shape, worst[torch.float32], compared[torch.float32], worst[torch.float64], compared[torch.float64]))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape,bound", [((4, 2, 5), "sliding"), ((6, 5), ["sliding", "dft"]), ((3, 3, 3), ["zero", "sliding", "dft"])], ids=str)
def test_converged_solution_is_the_dense_solve(shape, bound, dtype):
    dim = len(shape)
    g = field(shape, 700, dtype)
    h, Hd = st.hessian_arg(shape, 701, "full", dtype)
    L = el.dense(el.entries(shape, bound, VOXELS[dim], **FIVE))
    got, info = interpol.regulariser_solve(g.to(DEV), h.to(DEV), voxel_size=VOXELS[dim], bound=bound, max_iter=200, return_info=True, **FIVE)
    got = got.cpu().double()
    assert bool(torch.isfinite(got).all())
    for b in range(2):
        A = L + torch.block_diag(*Hd[b].reshape(-1, dim, dim))
        assert float((A - A.T).abs().max()) <= 1e-13 * float(A.abs().max())
        ev = torch.linalg.eigvalsh(A)
        assert float(ev[0]) > 0
        cond = float(ev[-1] / ev[0])
        want = torch.linalg.solve(A, g[b].double().reshape(-1)).reshape(g[b].shape)
        scale = float(want.abs().max())
        bar = TOL[dtype] * scale if dtype == torch.float64 else cond * 2.0 ** -23 * scale
        err = float((got[b] - want).abs().max())
        print("converged %s %s item %d: cond(A) = %.0f, error / bar = %.3g, iterations %d" % (shape, dtype, b, cond, err / bar, int(info.iterations[b])))
        assert err <= bar, (b, err / bar)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_solve_bits_do_not_depend_on_the_run_or_on_the_batch(dtype):
    for shape, kind in (((9, 5, 67), "full"), ((19, 11), "diag"), ((130,), "none"), ((6, 1, 7), "full")):
        dim = len(shape)
        g = field(shape, 40, dtype).to(DEV)
        h = st.hessian_arg(shape, 41, kind, dtype)[0]
        h = None if h is None else h.to(DEV)
        kw = dict(max_iter=12, tolerance=0., return_info=True, voxel_size=VOXELS[dim], bound="sliding", **FIVE)
        x, info = interpol.regulariser_solve(g, h, **kw)
        x2, info2 = interpol.regulariser_solve(g, h, **kw)
        assert torch.equal(x, x2) and torch.equal(info.iterations, info2.iterations) and torch.equal(info.residual, info2.residual)
        for b in range(2):
            xb, infob = interpol.regulariser_solve(g[b:b + 1], None if h is None else h[b:b + 1], **kw)
            assert torch.equal(xb[0], x[b]) and torch.equal(infob.residual[0], info.residual[b]), (shape, b)


def test_solve_refuses_a_non_symmetric_L_on_the_device():
    g = field((4, 5), 72, torch.float32).to(DEV)
    for bound in ("dct2", "dst2", ["sliding", "dct2"]):
        with pytest.raises(ValueError, match="symmetric"):
            interpol.regulariser_solve(g, bound=bound, shears=1.0)
        with pytest.raises(ValueError):                                  # ... and so does the library: INTERPOL_E_BOUND
            _hip.regulariser_solve(g, None, (0., 0., 0., 1., 0.), [1., 1.], interpol.autograd.regulariser_bound_codes(bound, 2), 2, 0.)


def test_graph_replay_gives_the_bits_of_eager():
    shape = (9, 5, 67)
    kw = dict(voxel_size=[2.0, 0.75, 1.5], bound="sliding", **FIVE)
    skw = dict(max_iter=10, tolerance=1e-2, return_info=True, **kw)
    gen = torch.Generator().manual_seed(9)
    v = torch.randn([2, *shape, 3], generator=gen).to(DEV)
    h = st.hessian_arg(shape, 41, "full", torch.float32)[0].to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                        # warm-up on the side stream (module loads)
        interpol.regulariser(v, **kw); interpol.regulariser_energy(v, **kw); interpol.regulariser_solve(v, h, **skw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = interpol.regulariser(v, **kw)
        E = interpol.regulariser_energy(v, **kw)
        x, info = interpol.regulariser_solve(v, h, **skw)
    for it in range(3):
        v.copy_(torch.randn(v.shape, generator=gen) * (1 + it))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, interpol.regulariser(v, **kw)), it
        assert torch.equal(E, interpol.regulariser_energy(v, **kw)), it
        xe, infoe = interpol.regulariser_solve(v, h, **skw)
        assert torch.equal(x, xe) and torch.equal(info.iterations, infoe.iterations) and torch.equal(info.residual, infoe.residual), it
        assert bool((info.iterations > 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# 5. memory contract
# ---------------------------------------------------------------------------------------------------------------------
WEIGHT_SETS = [(0.3, 0.7, 1.3, 0.6, 0.9), (0., 0., 0., 0.6, 0.9), (0., 0., 1., 0., 1.), (0.3, 0.7, 1.3, 0., 0.)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("misalign", [0, 1, 3])
def test_memory_contract(misalign, dtype):
    for shape in ((9, 5, 67), (1, 2, 3), (19, 11), (130,), (2, 1, 1), (6, 1, 7)):
        dim = len(shape)
        u = field(shape, 400 + dim, dtype)
        ud = u.to(DEV)
        h = st.hessian_arg(shape, 410 + dim, "full", dtype)[0]
        hd = h.to(DEV)
        for weights in WEIGHT_SETS:
            for bound in (7, 0, 6):
                b, vx = [bound] * dim, VOXELS[dim]
                if bound != 7 and not (weights[3] or weights[4]):
                    continue                                             # (the three-term entry points: their own module)
                run = lambda f, hh: (_hip.regulariser(f, weights, vx, b), _hip.regulariser_energy(f, weights, vx, b),
                                     *_hip.regulariser_solve(f, hh, weights, vx, b, 3, 0.))
                ref = run(ud, hd)
                assert all(bool(torch.isfinite(r).all()) for r in ref)
                with memguard.installed(_hip, misalign=misalign) as seam:
                    up = memguard.place(u, DEV, misalign=misalign)
                    hp = memguard.place(h, DEV, misalign=misalign)
                    out = run(up, hp)
                    torch.cuda.synchronize()
                    what = (shape, weights, bound, misalign)
                    assert len(seam.outputs()) == 4 and len(seam.workspaces()) == 2 and seam.workspace_was_written(), what
                    off = misalign * u.element_size()
                    assert out[0].data_ptr() % memguard.ALIGN == off and out[2].data_ptr() % memguard.ALIGN == off, what
                    assert up.data_ptr() % memguard.ALIGN == off, what
                    for t, r in zip(out, ref):
                        seam.assert_fully_written(t, r, what)
                        # no NaN from a read outside the field or from a stale workspace, and the very same values as from ordinary buffers
                        assert torch.equal(t, r), what
                    seam.assert_guards_intact(what)
                    memguard.assert_guard_intact(up, what)
                    memguard.assert_guard_intact(hp, what)
                    assert torch.equal(up, ud) and torch.equal(hp, hd), what


# ---------------------------------------------------------------------------------------------------------------------
# 6. the C ABI
# ---------------------------------------------------------------------------------------------------------------------
def five(*w):
    return (ctypes.c_double * 5)(*w)


def test_old_modes_through_the_new_entry_points_keep_their_bits():
    L = _hip.lib()
    null = ctypes.c_void_p(0)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    for shape in ((9, 5, 67), (19, 11), (130,), (1, 2, 3)):
        dim = len(shape)
        for dtype in (torch.float32, torch.float64):
            u = field(shape, 600 + dim, dtype).to(DEV)
            h = st.hessian_arg(shape, 601, "full", dtype)[0].to(DEV)
            vx = (ctypes.c_double * 3)(*(VOXELS[dim] + [1.] * (3 - dim)))
            for w in ((0.3, 0.7, 1.3), (0., 1., 0.), (0., 0., 1.), (2., 0., 0.), (2., 1., 0.), (2., 0., 1.), (0., 1., 1.)):
                for bound in (3, 6, 1):
                    b = [bound] * dim
                    old = (_hip.regulariser(u, w, VOXELS[dim], b), _hip.regulariser_energy(u, w, VOXELS[dim], b))
                    p = _hip._regulariser_problem(u, b, u.stride(0))
                    out, en = torch.empty_like(u), torch.empty(2, dtype=dtype, device=DEV)
                    ws = torch.empty(2 * 1024 * 8, dtype=torch.uint8, device=DEV)
                    assert L.interpol_regulariser_elastic_energy_workspace(ctypes.byref(p)) == ws.numel()
                    assert L.interpol_regulariser_elastic(ctypes.byref(p), ptr(u), ptr(out), five(*w, 0., 0.), vx, null) == 0
                    assert L.interpol_regulariser_elastic_energy(ctypes.byref(p), ptr(u), ptr(en), five(*w, 0., 0.), vx, ptr(ws), ws.numel(), null) == 0
                    torch.cuda.synchronize()
                    assert torch.equal(out, old[0]) and torch.equal(en, old[1]), (shape, dtype, w, bound)
                    if bound == 1:
                        continue
                    xo, io = _hip.regulariser_solve(u, h, w, VOXELS[dim], b, 5, 0.)
                    K = h.shape[-1]
                    n = L.interpol_regulariser_elastic_solve_workspace(ctypes.byref(p), K)
                    assert n == L.interpol_regulariser_solve_workspace(ctypes.byref(p), K) and n > 0
                    sw = torch.empty(n, dtype=torch.uint8, device=DEV)
                    x, info = torch.empty_like(u), torch.empty(2, 2, dtype=torch.float64, device=DEV)
                    assert L.interpol_regulariser_elastic_solve(ctypes.byref(p), ptr(u), ptr(h), K, h.stride(0), ptr(x), five(*w, 0., 0.), vx, 5, 0.,
                                                                ptr(info), ptr(sw), n, null) == 0
                    torch.cuda.synchronize()
                    assert torch.equal(x, xo) and torch.equal(info, io), (shape, dtype, w, bound)


def test_entry_points_validate_before_launching():
    L = _hip.lib()
    shp = (6, 5, 4)
    f = torch.randn(1, *shp, 3, device=DEV)
    sentinel = 4321.0
    out = torch.full([1, *shp, 3], sentinel, device=DEV)
    en = torch.full([1], sentinel, device=DEV)
    ws = torch.zeros(1024 * 8, dtype=torch.uint8, device=DEV)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    null = ctypes.c_void_p(0)
    vx = (ctypes.c_double * 3)(1., 1., 1.)
    good = five(0., 1., 1., 1., 1.)

    def problem(dtype=torch.float32, dstr=None, C=3, dim=3, bound=7):
        st_ = [f.stride(0), 1, *f.stride()[1:4]]
        bound = bound if isinstance(bound, list) else [bound] * 3
        return _hip.make_problem(dim, dtype, dtype, bound, [0] * 3, 1, 1, C, shp, shp, dstr or st_, [0] * 5, [out.stride(0)] + [0] * 6, 0)

    solve_ws = L.interpol_regulariser_elastic_solve_workspace(ctypes.byref(problem()), 0)
    assert solve_ws > 0
    sws = torch.zeros(solve_ws, dtype=torch.uint8, device=DEV)

    def three(p, fld=f, o=out, e=en, w=good, h=vx, work=ws):
        return (L.interpol_regulariser_elastic(ctypes.byref(p), ptr(fld), ptr(o), w, h, null),
                L.interpol_regulariser_elastic_energy(ctypes.byref(p), ptr(fld), ptr(e), w, h, ptr(work), work.numel(), null),
                L.interpol_regulariser_elastic_solve(ctypes.byref(p), ptr(fld), null, 0, 0, ptr(o), w, h, 2, 0., null, ptr(sws), sws.numel(), null))

    # the old entry points do not know the sliding code
    p7 = problem(bound=7)
    assert L.interpol_regulariser(ctypes.byref(p7), ptr(f), ptr(out), 0., 1., 1., vx, null) == -3
    assert L.interpol_regulariser_energy(ctypes.byref(p7), ptr(f), ptr(en), 0., 1., 1., vx, ptr(ws), ws.numel(), null) == -3
    assert L.interpol_regulariser_energy_workspace(ctypes.byref(p7)) == -3 and L.interpol_regulariser_solve_workspace(ctypes.byref(p7), 0) == -3
    assert L.interpol_regulariser_solve(ctypes.byref(p7), ptr(f), null, 0, 0, ptr(out), 0., 1., 1., vx, 2, 0., null, ptr(sws), sws.numel(), null) == -3
    assert L.interpol_regulariser_elastic_energy_workspace(ctypes.byref(p7)) == 1024 * 8
    assert three(problem(bound=8)) == (-3, -3, -3)                      # INTERPOL_E_BOUND
    assert three(problem(bound=-1)) == (-3, -3, -3)
    assert three(problem(dtype=torch.bfloat16)) == (-4, -4, -4)         # INTERPOL_E_DTYPE
    assert three(problem(dstr=[f.stride(0), 120, 20, 4, 1])) == (-10, -10, -10)   # a channel-first field: INTERPOL_E_STRIDE
    assert three(problem(C=2)) == (-5, -5, -5)                          # components != dims: INTERPOL_E_SHAPE
    for bad in (five(0., 1., 1., -1., 1.), five(0., 1., 1., 1., -1.), five(0., 0., 0., float("nan"), 0.), five(0., 0., 0., 0., float("inf")),
                five(0., 0., 0., 0., 0.)):
        assert three(problem(), w=bad) == (-5, -5, -5)                  # a negative or non-finite weight, or no term at all
    assert three(problem(), h=(ctypes.c_double * 3)(1., 0., 1.)) == (-5, -5, -5)
    assert three(problem(), w=None) == (-6, -6, -6)                     # INTERPOL_E_NULL
    # elastic terms in the solve under a bound that is not symmetric: the matvec and the energy run, the solve refuses
    for b in (3, 5, 1, [7, 3, 7]):
        assert L.interpol_regulariser_elastic_solve(ctypes.byref(problem(bound=b)), ptr(f), null, 0, 0, ptr(out), good, vx, 2, 0., null,
                                                    ptr(sws), sws.numel(), null) == -3
    assert L.interpol_regulariser_elastic_solve_workspace(ctypes.byref(problem(bound=1)), 0) == -3
    # overlap rules as today
    assert L.interpol_regulariser_elastic(ctypes.byref(problem()), ptr(f), ptr(f), good, vx, null) == -10
    inside = f.view(-1)[7:]
    assert L.interpol_regulariser_elastic_energy(ctypes.byref(problem()), ptr(f), ptr(inside), good, vx, ptr(ws), ws.numel(), null) == -10
    assert L.interpol_regulariser_elastic_energy(ctypes.byref(problem()), ptr(f), ptr(en), good, vx, ptr(ws), 1024 * 8 - 1, null) == -9
    assert L.interpol_regulariser_elastic_solve(ctypes.byref(problem()), ptr(f), null, 0, 0, ptr(f), good, vx, 2, 0., null, ptr(sws), sws.numel(), null) == -10
    assert L.interpol_regulariser_elastic_solve(ctypes.byref(problem()), ptr(f), null, 0, 0, ptr(out), good, vx, 2, 0., null, ptr(sws), sws.numel() - 1, null) == -9
    torch.cuda.synchronize()
    assert bool((out == sentinel).all()) and bool((en == sentinel).all()) and not bool(ws.any()) and not bool(sws.any())
    assert three(problem()) == (0, 0, 0)
    # without elastic weights dct2 serves the solve through the new entry point too
    assert L.interpol_regulariser_elastic_solve(ctypes.byref(problem(bound=[7, 3, 5])), ptr(f), null, 0, 0, ptr(out), five(0., 1., 1., 0., 0.), vx, 2, 0.,
                                                null, ptr(sws), sws.numel(), null) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and not bool((out == sentinel).any()) and float(en) > 0 and float(en) != sentinel
