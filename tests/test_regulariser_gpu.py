"""`interpol.regulariser` / `interpol.regulariser_energy` on the device (csrc/regulariser.hip).

Truth: the dense float64 matrix of L assembled in tests/test_regulariser_cpu.py from the oracle's bound tables (`spatial_matrix`,
`apply_dense`, `energy_dense`), applied to the field as the device sees it (rounded to its dtype) -- never the code under test.

Bars.  L v on randn fields: |got - want| <= tol |want| + tol max|want|, tol = 1e-5 (float32) / 1e-11 (float64) / 1e-2 (bf16
storage).  Energy: rtol = tol, with absolute > 0 so that the energy is well away from zero.  Gradients: the L v bar against
L^T g, resp. g 0.5 (L + L^T) v.  Smooth fields (float32): the a-priori bound n 2^-24 ||L||_inf max|v| (see the test).

Shapes: the smallest that can still break the kernels.  A workgroup of reg_fwd owns 256 lattice points in storage order, in
every D: (9, 5, 67) has 3015 points -- twelve workgroups that straddle rows and planes, the last one ragged; (130,) and
(19, 11) end inside a workgroup; at (3, 3, 3), (1, 2, 3), (2, 1, 1) and (4, 2, 5) the 2-ring stencil is wider than the volume
and taps wrap more than once.  The energy kernel runs 1024 persistent workgroups per item whatever the shape.  The shipped
organisation is one thread per lattice point (no LDS tile), so there is no tile shape to straddle.  B = 2 everywhere.
"""
import ctypes

import pytest
import torch

import interpol
from interpol import _hip, backend, ops
import memguard
import test_regulariser_cpu as truth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = {torch.float32: 1e-5, torch.float64: 1e-11, torch.bfloat16: 1e-2}
BOUNDS = truth.BOUNDS
SYMMETRIC = truth.SYMMETRIC
SHAPES = [(130,), (19, 11), (9, 5, 67), (3, 3, 3), (1, 2, 3), (2, 1, 1), (4, 2, 5)]
IDS = ["x".join(map(str, s)) for s in SHAPES]
VOXELS = {1: [1.5], 2: [0.5, 1.25], 3: [2.0, 0.75, 1.5]}
ALL = dict(absolute=2.0, membrane=0.7, bending=0.3)
# (weights, bound, anisotropic): all seven bounds for membrane + bending together, each term alone on dft and dct2, one anisotropic
CASES = ([(dict(membrane=0.7, bending=1.3), b, False) for b in BOUNDS]
         + [(w, b, False) for b in ("dft", "dct2") for w in (dict(absolute=2.0), dict(membrane=1.0), dict(bending=1.0))]
         + [(dict(absolute=0.3, membrane=0.7, bending=1.3), "dct2", True)])

field = truth.field
assert_close = truth.assert_close


def fused_calls(monkeypatch):
    """count the calls that reach the entry points of the library"""
    calls = dict(matvec=0, energy=0)
    mv, en = _hip.regulariser, _hip.regulariser_energy

    def f(*a, **k):
        calls["matvec"] += 1
        return mv(*a, **k)

    def e(*a, **k):
        calls["energy"] += 1
        return en(*a, **k)

    monkeypatch.setattr(_hip, "regulariser", f)
    monkeypatch.setattr(_hip, "regulariser_energy", e)
    return calls


# ---------------------------------------------------------------------------------------------------------------------
# 5. forward against the dense matrix
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", range(len(SHAPES)), ids=IDS)
def test_forward_matches_the_dense_matrix(case, dtype, monkeypatch):
    shape = SHAPES[case]
    dim = len(shape)
    v = field(shape, 100 + case, dtype)
    vd = v.to(DEV)
    calls = fused_calls(monkeypatch)
    mixed = ["dct2", "dst1", "zero"][:dim]
    for w, bound, aniso in CASES + [(dict(membrane=0.7, bending=1.3), mixed, False)]:
        vx = VOXELS[dim] if aniso else 1.
        S = truth.spatial_matrix(shape, bound, voxel_size=vx, **w)
        want = truth.apply_dense(S, v, vx)
        assert float(want.abs().max()) > 0.1 * float(v.abs().max())     # (randn: the bar is not vacuous)
        for B in (2, 1):
            assert ops.regulariser_covered(vd[:B])
            got = interpol.regulariser(vd[:B], voxel_size=vx, bound=bound, **w)
            assert got.dtype == dtype
            assert_close(got, want[:B], TOL[dtype], (shape, w, bound, vx, B))
    assert calls["matvec"] == 2 * (len(CASES) + 1) and calls["energy"] == 0


# ---------------------------------------------------------------------------------------------------------------------
# 6. smooth fields: the a-priori bound
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
    """float32, |got - want| <= n 2^-24 ||L||_inf max|v| with n = 32, the longest chain of rounded operations of reg_at
    (csrc/regulariser.hip) behind one output, in 3-D with all three terms: the coefficient tables are rounded once from
    double (1); the centre coefficient is three additions or three fused multiply-adds of products of A's taps, then one
    fused multiply-add with 2 bending (4); the centre product (1); 12 fused multiply-adds along the axes and 12 for the
    diagonals (24); the product with h_d^2 and the rounding of h_d^2 itself (2).  Signs are exact.  The coefficient of a
    later tap has a shorter chain of its own (at most 4) and fewer accumulations behind it.  Fewer terms or dimensions
    only shorten the chain.  ||L||_inf comes from the dense matrix; it bounds sum |coefficient| |v| of every row."""
    n = 32
    dim = len(shape)
    v = smooth_field(shape).float()
    vd = v.to(DEV)
    worst = 0.0
    for w in (dict(membrane=1.0), dict(bending=1.0), dict(absolute=0.3, membrane=0.7, bending=1.3)):
        for bound, vx in (("dft", 1.), ("dct2", 1.), ("dft", VOXELS[dim])):
            S = truth.spatial_matrix(shape, bound, voxel_size=vx, **w)
            want = truth.apply_dense(S, v, vx)
            bar = n * 2.0 ** -24 * truth.norm_inf(S, dim, vx) * float(v.abs().max())
            got = interpol.regulariser(vd, voxel_size=vx, bound=bound, **w).cpu().double()
            ratio = float((got - want).abs().max()) / bar
            small = float(want.abs().max()) / (truth.norm_inf(S, dim, vx) * float(v.abs().max()))
            print("smooth %s %s %s vx=%s: max|want| / (||L|| max|v|) = %.3g, error / bound = %.4f" % (shape, w, bound, vx, small, ratio))
            worst = max(worst, ratio)
            assert ratio <= 1.0, (shape, w, bound, vx, ratio)
    print("smooth %s: worst error / bound = %.4f" % (shape, worst))


# ---------------------------------------------------------------------------------------------------------------------
# 7. energy
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", range(len(SHAPES)), ids=IDS)
def test_energy_matches_the_dense_matrix(case, dtype, monkeypatch):
    shape = SHAPES[case]
    dim = len(shape)
    v = field(shape, 200 + case, dtype)
    vd = v.to(DEV)
    calls = fused_calls(monkeypatch)
    n = 0
    for w, bound, vx in ((ALL, "dft", 1.), (ALL, "dct2", VOXELS[dim]), (ALL, "replicate", 1.), (ALL, "dst1", 1.),
                         (dict(absolute=2.0), "dft", 1.), (dict(absolute=2.0, membrane=1.0), "zero", 1.),
                         (dict(absolute=2.0, bending=1.0), "dst2", 1.)):
        S = truth.spatial_matrix(shape, bound, voxel_size=vx, **w)
        want = truth.energy_dense(S, v, vx)
        assert bool((want > 0.1 * v.double().square().reshape(2, -1).sum(1)).all())          # (well away from zero)
        kw = dict(voxel_size=vx, bound=bound, **w)
        E = interpol.regulariser_energy(vd, **kw)
        assert E.shape == (2,) and E.dtype == dtype
        rel = ((E.cpu().double() - want).abs() / want.abs())
        assert bool((rel <= TOL[dtype]).all()), (shape, w, bound, vx, float(rel.max()))
        # two identical calls give identical bits, and an item gives the same bits alone and inside the batch
        assert torch.equal(E, interpol.regulariser_energy(vd, **kw))
        assert torch.equal(E[:1], interpol.regulariser_energy(vd[:1], **kw))
        assert torch.equal(E[1:], interpol.regulariser_energy(vd[1:], **kw))
        n += 4
    assert calls["energy"] == n and calls["matvec"] == 0


# ---------------------------------------------------------------------------------------------------------------------
# 8. backward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", [(130,), (19, 11), (9, 5, 67), (1, 2, 3)], ids=["1d", "2d", "3d", "tiny"])
def test_backward_is_the_transposed_matrix(shape, dtype, monkeypatch):
    dim = len(shape)
    w = dict(absolute=0.3, membrane=0.7, bending=1.3)
    v = field(shape, 300 + dim, dtype)
    g = field(shape, 310 + dim, dtype)
    ge = torch.tensor([0.7, -1.9], dtype=torch.float64).to(dtype)
    calls = fused_calls(monkeypatch)
    for bound in BOUNDS + [["dct2", "dft", "zero"][:dim]]:
        symmetric = all(b in SYMMETRIC for b in ([bound] if isinstance(bound, str) else bound))
        vx = VOXELS[dim]
        S = truth.spatial_matrix(shape, bound, voxel_size=vx, **w)
        kw = dict(voxel_size=vx, bound=bound, **w)
        x = v.to(DEV).requires_grad_()
        before = dict(calls)
        got, = torch.autograd.grad(interpol.regulariser(x, **kw), x, g.to(DEV))
        # the forward always reaches the fused kernel; the backward does where L is symmetric and must not where it is not
        assert calls["matvec"] - before["matvec"] == (2 if symmetric else 1), bound
        assert_close(got, truth.apply_dense(S, g, vx, transpose=True), TOL[dtype], ("matvec", shape, bound))
        before = dict(calls)
        got, = torch.autograd.grad(interpol.regulariser_energy(x, **kw), x, ge.to(DEV))
        assert (calls["energy"] - before["energy"], calls["matvec"] - before["matvec"]) == (1, 1 if symmetric else 0), bound
        want = 0.5 * (truth.apply_dense(S, v, vx) + truth.apply_dense(S, v, vx, transpose=True)) * ge.double().reshape([2] + [1] * (dim + 1))
        assert_close(got, want, TOL[dtype], ("energy", shape, bound))


@pytest.mark.parametrize("bound", ["dct2", "dft", "replicate", "dst1"])
def test_gradcheck_on_the_device(bound, monkeypatch):
    kw = dict(absolute=0.3, membrane=0.7, bending=1.3, voxel_size=[2.0, 0.75, 1.5], bound=bound)
    v = field((4, 3, 5), 33, B=1).to(DEV).requires_grad_()
    calls = fused_calls(monkeypatch)
    assert torch.autograd.gradcheck(lambda x: interpol.regulariser(x, **kw), (v,))
    assert torch.autograd.gradcheck(lambda x: interpol.regulariser_energy(x, **kw), (v,))
    assert calls["matvec"] > 0 and calls["energy"] > 0


def test_double_backward_on_the_device():
    """L is linear: the second derivative of sum (L v)^2 is 2 L^T L, every application of L on the fused kernel"""
    shape, bound = (4, 3, 5), "dct2"
    w = dict(membrane=0.7, bending=1.3)
    S = truth.spatial_matrix(shape, bound, **w)
    v = field(shape, 34).to(DEV).requires_grad_()
    g1, = torch.autograd.grad(interpol.regulariser(v, bound=bound, **w).square().sum(), v, create_graph=True)
    z = field(shape, 35)
    g2, = torch.autograd.grad(g1, v, z.to(DEV))
    want = 2 * truth.apply_dense(S, truth.apply_dense(S, z), transpose=True)
    assert_close(g2, want, 1e-11, "double backward")


# ---------------------------------------------------------------------------------------------------------------------
# 9. routing
# ---------------------------------------------------------------------------------------------------------------------
def test_default_routing_is_the_fused_kernel(monkeypatch):
    assert backend.fused_regulariser is True
    calls = fused_calls(monkeypatch)
    for shape in ((130,), (19, 11), (9, 5, 67)):
        for dtype in (torch.float32, torch.float64):
            vd = field(shape, 1, dtype).to(DEV)
            assert ops.regulariser_covered(vd)
            before = dict(calls)
            interpol.regulariser(vd, membrane=1.)
            interpol.regulariser_energy(vd, membrane=1.)
            assert (calls["matvec"] - before["matvec"], calls["energy"] - before["energy"]) == (1, 1)
    # all weights zero: zeros, and nothing is launched
    before = dict(calls)
    assert not bool(interpol.regulariser(vd).any()) and not bool(interpol.regulariser_energy(vd).any())
    assert calls == before


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
    w = dict(absolute=2.0, membrane=0.7, bending=0.3)
    S = truth.spatial_matrix(shape, "dct2", **w)
    got = interpol.regulariser(vd, bound="dct2", **w)
    E = interpol.regulariser_energy(vd, bound="dct2", **w)
    assert calls == dict(matvec=0, energy=0) and got.dtype == dtype and E.dtype == dtype
    # (16-bit: the truth sees the rounded values)
    assert_close(got.float(), truth.apply_dense(S, v.float()), TOL[dtype], what)
    want = truth.energy_dense(S, v.float())
    assert bool(((E.cpu().double() - want).abs() <= TOL[dtype] * want.abs()).all()), what
    if what != "bf16":
        x = vd.clone().requires_grad_()
        g, = torch.autograd.grad(interpol.regulariser_energy(x, bound="dct2", **w).sum(), x)
        assert_close(g, truth.apply_dense(S, v), TOL[dtype], what)
        assert calls == dict(matvec=0, energy=0)


# ---------------------------------------------------------------------------------------------------------------------
# 10. memory contract
# ---------------------------------------------------------------------------------------------------------------------
WEIGHT_SETS = [(0.3, 0.7, 1.3), (0., 1., 0.), (0., 0., 1.), (2., 0., 0.)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("misalign", [0, 1, 3])
def test_memory_contract(misalign, dtype):
    for shape in ((9, 5, 67), (1, 2, 3), (19, 11), (130,), (2, 1, 1)):
        dim = len(shape)
        u = field(shape, 400 + dim, dtype)
        ud = u.to(DEV)
        for weights in WEIGHT_SETS:
            for bound in (3, 6, 0, 4):
                b, vx = [bound] * dim, VOXELS[dim]
                ref = (_hip.regulariser(ud, weights, vx, b), _hip.regulariser_energy(ud, weights, vx, b))
                assert all(bool(torch.isfinite(r).all()) for r in ref)
                with memguard.installed(_hip, misalign=misalign) as seam:
                    up = memguard.place(u, DEV, misalign=misalign)
                    out = (_hip.regulariser(up, weights, vx, b), _hip.regulariser_energy(up, weights, vx, b))
                    torch.cuda.synchronize()
                    what = (shape, weights, bound, misalign)
                    assert len(seam.outputs()) == 2 and len(seam.workspaces()) == 1 and seam.workspace_was_written(), what
                    assert out[0].shape == u.shape and out[1].shape == (2,), what
                    off = misalign * u.element_size()
                    assert out[0].data_ptr() % memguard.ALIGN == off and up.data_ptr() % memguard.ALIGN == off, what
                    for t, r in zip(out, ref):
                        seam.assert_fully_written(t, r, what)
                        # no NaN from a read outside the field or from a stale workspace, and the very same values as from ordinary buffers
                        assert torch.equal(t, r), what
                    seam.assert_guards_intact(what)
                    memguard.assert_guard_intact(up, what)
                    assert torch.equal(up, ud), what


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_views_with_an_offset_and_strided_fields(dim):
    shape = {1: (130,), 2: (19, 11), 3: (9, 5, 67)}[dim]
    u = field(shape, 500 + dim, torch.float32).to(DEV)
    weights, vx, b = (0.3, 0.7, 1.3), VOXELS[dim], [3] * dim
    ref = (_hip.regulariser(u, weights, vx, b), _hip.regulariser_energy(u, weights, vx, b))
    # a view whose storage starts one element into its buffer
    buf = torch.full([u.numel() + 1], float("nan"), device=DEV)
    view = buf[1:].view(u.shape)
    view.copy_(u)
    assert view.storage_offset() == 1 and view.data_ptr() % 8 != 0
    # a field stored channel-first (not point by point), and every other item of a larger batch
    chan = u.movedim(-1, 1).contiguous().movedim(1, -1)
    assert dim == 1 or not chan.is_contiguous()
    wide = torch.stack([u, u + 1], 1)[:, 0]
    assert wide.stride(0) == 2 * u.stride(0)
    for v in (view, chan, wide):
        got = (_hip.regulariser(v, weights, vx, b), _hip.regulariser_energy(v, weights, vx, b))
        for t, r in zip(got, ref):
            assert torch.equal(t, r), dim
        assert torch.equal(interpol.regulariser(v, 0.3, 0.7, 1.3, vx, "dct2"), ref[0])
        assert torch.equal(interpol.regulariser_energy(v, 0.3, 0.7, 1.3, vx, "dct2"), ref[1])
    with pytest.raises(ValueError):
        _hip.regulariser(u, weights, vx, b, out=u)                     # the output is the field


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

    def problem(dtype=torch.float32, dstr=None, C=3, dim=3, bound=3):
        st = [f.stride(0), 1, *f.stride()[1:4]]
        return _hip.make_problem(dim, dtype, dtype, [bound] * 3, [0] * 3, 1, 1, C, shp, shp, dstr or st, [0] * 5, [out.stride(0)] + [0] * 6, 0)

    def both(p, fld=f, o=out, e=en, w=(0., 1., 1.), h=vx, work=ws):
        return (L.interpol_regulariser(ctypes.byref(p), ptr(fld), ptr(o), *w, h, null),
                L.interpol_regulariser_energy(ctypes.byref(p), ptr(fld), ptr(e), *w, h, ptr(work), work.numel(), null))

    assert L.interpol_regulariser_energy_workspace(ctypes.byref(problem())) == 1024 * 8
    assert both(problem(dtype=torch.bfloat16)) == (-4, -4)              # INTERPOL_E_DTYPE
    assert both(problem(dtype=torch.float16)) == (-4, -4)
    assert both(problem(dstr=[f.stride(0), 120, 20, 4, 1])) == (-10, -10)     # a channel-first field: INTERPOL_E_STRIDE
    assert both(problem(C=2)) == (-5, -5)                               # components != dims: INTERPOL_E_SHAPE
    assert both(problem(bound=7)) == (-3, -3)                           # INTERPOL_E_BOUND
    assert both(problem(), w=(0., -1., 1.)) == (-5, -5)                 # a negative weight
    assert both(problem(), w=(0., 0., 0.)) == (-5, -5)                  # no term at all
    assert both(problem(), h=(ctypes.c_double * 3)(1., 0., 1.)) == (-5, -5)   # a voxel size that is not positive
    # overlapping input and output: the output is the field, starts inside it, or the energy / the workspace lies inside it
    assert L.interpol_regulariser(ctypes.byref(problem()), ptr(f), ptr(f), 0., 1., 1., vx, null) == -10
    inside = f.view(-1)[7:]
    assert L.interpol_regulariser(ctypes.byref(problem()), ptr(f), ptr(inside), 0., 1., 1., vx, null) == -10
    assert L.interpol_regulariser_energy(ctypes.byref(problem()), ptr(f), ptr(inside), 0., 1., 1., vx, ptr(ws), ws.numel(), null) == -10
    assert L.interpol_regulariser_energy(ctypes.byref(problem()), ptr(f), ptr(en), 0., 1., 1., vx, ptr(ws), 1024 * 8 - 1, null) == -9   # INTERPOL_E_SCRATCH
    assert L.interpol_regulariser(ctypes.byref(problem()), null, ptr(out), 0., 1., 1., vx, null) == -6
    assert L.interpol_regulariser_energy(ctypes.byref(problem()), ptr(f), ptr(en), 0., 1., 1., vx, null, 0, null) == -6
    torch.cuda.synchronize()
    assert bool((out == sentinel).all()) and bool((en == sentinel).all()) and not bool(ws.any()) and bool(torch.isfinite(f).all())
    assert both(problem()) == (0, 0)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and not bool((out == sentinel).any()) and float(en) > 0 and float(en) != sentinel


# ---------------------------------------------------------------------------------------------------------------------
# 11. hipGraph capture
# ---------------------------------------------------------------------------------------------------------------------
def test_graph_replay_gives_the_bits_of_eager():
    kw = dict(absolute=0.3, membrane=0.7, bending=1.3, voxel_size=[2.0, 0.75, 1.5], bound="dct2")
    gen = torch.Generator().manual_seed(9)
    v = torch.randn([2, 9, 5, 67, 3], generator=gen).to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                        # warm-up on the side stream (module loads)
        interpol.regulariser(v, **kw); interpol.regulariser_energy(v, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = interpol.regulariser(v, **kw)
        E = interpol.regulariser_energy(v, **kw)
    for it in range(3):
        v.copy_(torch.randn(v.shape, generator=gen) * (1 + it))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, interpol.regulariser(v, **kw)), it
        assert torch.equal(E, interpol.regulariser_energy(v, **kw)), it
