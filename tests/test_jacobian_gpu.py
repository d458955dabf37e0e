"""`interpol.jacobian` / `interpol.jacdet` on the device (csrc/jacobian.hip).

Definition everywhere: jacobian(u) = grid_grad(u channel-first, identity_grid(shape), extrapolate=True) moved to (..., D, D), plus
the identity; jacdet = its determinant.  Forward truth: the C oracle on the CPU in the field's dtype, compared in float64;
backward truth: the float64 composed route on the device, differentiated by autograd through the existing operators -- never
the code under test.

Fields are plain randn: the sample points are the lattice points, exact in every dtype.

Bars.  Forward: |got - want| <= tol |want| + tol max|want|, tol = 1e-5 (float32) / 1e-11 (float64) / 1e-2 (bf16 storage).
Backward: rtol = tol, atol = tol max|ref| per gradient.

Shapes: the smallest that can still break the kernels.  A workgroup owns 256 lattice points in storage order, in every D:
(9, 5, 67) has 3015 points -- twelve workgroups that straddle rows and planes, the last one ragged; (130,) and (19, 11) end
inside a workgroup; (3, 3, 3), (1, 2, 3) and (2, 1, 1) are the extents at which the stencil is wider than the volume and taps
fold onto each other.

Routing: the library instantiates orders 1, 2 and 3; `interpol.backend.fused_jacobian_orders` decides which of them the host
layer sends there.  The tests below run with all three routed to the fused kernels, so that every instantiation is held to the
bars; one test checks the default.
"""
import ctypes

import pytest
import torch

import interpol
from interpol import _hip, backend, ops
from interpol.torch_kernels import det_closed
from oracle import oracle
import memguard

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = {torch.float32: 1e-5, torch.float64: 1e-11, torch.bfloat16: 1e-2}
BOUNDS = ["zero", "replicate", "dct1", "dct2", "dst1", "dst2", "dft"]
SHAPES = [(130,), (19, 11), (9, 5, 67), (3, 3, 3), (1, 2, 3), (2, 1, 1)]
IDS = ["x".join(map(str, s)) for s in SHAPES]
# (order, bound code): all seven bounds for order 1; dct2, dft, zero, dst1 for orders 2 - 3
STENCILS = [(1, b) for b in range(7)] + [(k, b) for k in (2, 3) for b in (3, 6, 0, 4)]


@pytest.fixture(autouse=True)
def every_instantiated_order_fused(monkeypatch):
    monkeypatch.setattr(backend, "fused_jacobian_orders", (1, 2, 3))


def field(shape, seed, dtype, B=2):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn([B, *shape, len(shape)], generator=gen, dtype=torch.float64).to(dtype)


_TRUTH = {}


def oracle_jacobian(u, bound, order, key=None):
    """oracle.grid_grad(u channel-first, identity_grid) + identity in the dtype of u (a CPU tensor), as float64; bound: one code or a
    per-dim list.  `key`: computed once per (field, stencil) and shared by the tests that need it."""
    if key is not None and (key, str(bound), str(order)) in _TRUTH:
        return _TRUTH[(key, str(bound), str(order))]
    dim = u.shape[-1]
    shape = u.shape[1:-1]
    grid = interpol.identity_grid(shape, dtype=u.dtype)[None].expand(u.shape[0], *shape, dim).contiguous()
    bound_list = bound if isinstance(bound, list) else [bound] * dim
    g = torch.as_tensor(oracle.grid_grad(u.movedim(-1, 1).contiguous(), grid, bound_list, order, 1))
    want = (g.movedim(1, -2) + torch.eye(dim, dtype=u.dtype)).double()
    if key is not None:
        _TRUTH[(key, str(bound), str(order))] = want
    return want


def oracle_det(u, bound, order, key=None):
    """the determinant of the oracle's Jacobian, expanded in the dtype of u, as float64"""
    return det_closed(oracle_jacobian(u, bound, order, key).to(u.dtype)).double()


def assert_close(got, want, tol, what):
    got = got.detach().cpu().double()
    err = (got - want).abs()
    allow = tol * want.abs() + tol * float(want.abs().max())
    assert got.shape == want.shape and bool(torch.isfinite(got).all()), what
    assert bool((err <= allow).all()), (what, float((err / allow.clamp_min(1e-300)).max()))


def fused_calls(monkeypatch):
    """count the calls that reach the entry points of the library"""
    calls = dict(fwd=0, field=0)
    fwd, fld = _hip.jacobian, _hip.jacdet_backward_field

    def f(*a, **k):
        calls["fwd"] += 1
        return fwd(*a, **k)

    def b(*a, **k):
        calls["field"] += 1
        return fld(*a, **k)

    monkeypatch.setattr(_hip, "jacobian", f)
    monkeypatch.setattr(_hip, "jacdet_backward_field", b)
    return calls


# ---------------------------------------------------------------------------------------------------------------------
# 1. forward parity against the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", range(len(SHAPES)), ids=IDS)
def test_forward_matches_the_oracle(case, dtype, monkeypatch):
    shape = SHAPES[case]
    dim = len(shape)
    u = field(shape, 100 + case, dtype)
    ud = u.to(DEV)
    calls = fused_calls(monkeypatch)
    n = 0
    mixed = [[3, 6, 0][d % 3] for d in range(dim)] if dim > 1 else [4]
    for order, bound in STENCILS + [(3, mixed), (1, mixed)]:
        names = [BOUNDS[b] for b in bound] if isinstance(bound, list) else BOUNDS[bound]
        kw = dict(interpolation=order, bound=names)
        for B in (2, 1):
            assert ops.jacobian_covered(ud[:B], [order])
            key = (case, dtype, B)
            what = (shape, order, bound, B)
            J = interpol.jacobian(ud[:B], **kw)
            assert J.dtype == dtype
            assert_close(J, oracle_jacobian(u[:B], bound, order, key), TOL[dtype], ("jacobian",) + what)
            d = interpol.jacdet(ud[:B], **kw)
            assert d.dtype == dtype
            assert_close(d, oracle_det(u[:B], bound, order, key), TOL[dtype], ("jacdet",) + what)
            n += 2
    # without the identity
    J0 = interpol.jacobian(ud, interpolation=3, bound="dct2", add_identity=False)
    assert_close(J0, oracle_jacobian(u, 3, 3, (case, dtype, 2)) - torch.eye(dim, dtype=torch.float64), TOL[dtype], "add_identity=False")
    assert calls["fwd"] == n + 1            # every call went through interpol_jacobian


# ---------------------------------------------------------------------------------------------------------------------
# 2. the two forward kernels share one J
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_jacdet_is_the_determinant_of_the_fused_jacobian(dtype):
    for case, shape in enumerate(SHAPES):
        ud = field(shape, 150 + case, dtype).to(DEV)
        for order, bound in STENCILS:
            kw = dict(interpolation=order, bound=BOUNDS[bound])
            want = det_closed(interpol.jacobian(ud, **kw).double()).cpu()
            assert_close(interpol.jacdet(ud, **kw), want, TOL[dtype], (shape, order, bound))


# ---------------------------------------------------------------------------------------------------------------------
# 3. backward parity against the float64 composed route on the device
# ---------------------------------------------------------------------------------------------------------------------
def composed_jacobian(u, **kw):
    """through the public grid_grad, as a user without this feature writes it"""
    dim = u.shape[-1]
    return interpol.grid_grad(u.movedim(-1, 1), torch.zeros_like(u), displacement=True, extrapolate=True, **kw).movedim(1, -2) \
        + torch.eye(dim, dtype=u.dtype, device=u.device)


def assert_grad(got, ref, tol, what):
    err = (got.double() - ref).abs()
    allow = tol * ref.abs() + tol * float(ref.abs().max())
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), what
    assert bool((err <= allow).all()), (what, float((err / allow.clamp_min(1e-300)).max()))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", range(len(SHAPES)), ids=IDS)
def test_backward_matches_the_composed_route(case, dtype, monkeypatch):
    shape = SHAPES[case]
    dim = len(shape)
    ud = field(shape, 200 + case, dtype).to(DEV)
    gen = torch.Generator().manual_seed(case)
    w = torch.randn(ud.shape[:-1], generator=gen, dtype=torch.float64).to(DEV)
    W = torch.randn([*ud.shape, dim], generator=gen, dtype=torch.float64).to(DEV)
    calls = fused_calls(monkeypatch)
    n = 0
    for order in (1, 2, 3):
        for bound in ("dct2", "dft", "zero", "dst1"):
            kw = dict(interpolation=order, bound=bound)
            for B in (2, 1):
                r = ud[:B].double().requires_grad_()
                Jr = composed_jacobian(r, **kw)
                ref_d, = torch.autograd.grad((torch.linalg.det(Jr) * w[:B]).sum(), r, retain_graph=True)
                ref_J, = torch.autograd.grad((Jr * W[:B]).sum(), r)
                v = ud[:B].clone().requires_grad_()
                got_d, = torch.autograd.grad((interpol.jacdet(v, **kw) * w[:B].to(dtype)).sum(), v)
                got_J, = torch.autograd.grad((interpol.jacobian(v, **kw) * W[:B].to(dtype)).sum(), v)
                n += 1
                if bound == "dft" and all(m == 1 or (m == 2 and order >= 2) for m in shape):
                    # Every derivative stencil cancels identically here (an extent of 1, or o - 1 = o + 1 in a period of 2): J = I,
                    # and both gradients are sums of +-1/2 w (+-1/2 W) that are zero in exact arithmetic.  The reference holds its own
                    # rounding noise, to which no relative bar applies: the bar is relative to the terms that cancel.
                    assert float(ref_d.abs().max()) <= 1e-14 * float(w.abs().max()) and float(ref_J.abs().max()) <= 1e-14 * float(W.abs().max())
                    assert float(got_d.abs().max()) <= TOL[dtype] * float(w.abs().max()), (shape, order, bound, B)
                    assert float(got_J.abs().max()) <= TOL[dtype] * float(W.abs().max()), (shape, order, bound, B)
                    continue
                assert_grad(got_d, ref_d, TOL[dtype], ("jacdet", shape, order, bound, B))
                assert_grad(got_J, ref_J, TOL[dtype], ("jacobian", shape, order, bound, B))
    assert calls["field"] == n and calls["fwd"] == 2 * n


def test_double_backward_matches_the_composed_route():
    ud = field((6, 5, 7), 31, torch.float64, B=1).to(DEV)
    kw = dict(interpolation=3, bound="dct2")
    res = []
    for f in (lambda v: interpol.jacdet(v, **kw), lambda v: torch.linalg.det(composed_jacobian(v, **kw))):
        v = ud.clone().requires_grad_()
        g1, = torch.autograd.grad(f(v).square().sum(), v, create_graph=True)
        res.append(torch.autograd.grad(g1.square().sum(), v)[0])
    assert bool(torch.isfinite(res[0]).all())
    assert float((res[0] - res[1]).abs().max()) <= 1e-9 * float(res[1].abs().max())


def test_gradcheck_runs_the_fused_kernels(monkeypatch):
    u = field((3, 2, 4), 17, torch.float64, B=1).to(DEV).requires_grad_()
    calls = fused_calls(monkeypatch)
    assert torch.autograd.gradcheck(lambda v: interpol.jacdet(v, interpolation=3, bound="dct2"), (u,))
    assert torch.autograd.gradcheck(lambda v: interpol.jacobian(v, interpolation=2, bound="dft"), (u,))
    assert calls["fwd"] > 0 and calls["field"] > 0


# ---------------------------------------------------------------------------------------------------------------------
# 4. routing
# ---------------------------------------------------------------------------------------------------------------------
def test_default_routing_sends_the_listed_orders_to_the_fused_kernels(monkeypatch):
    monkeypatch.undo()                                                   # (the package's own default)
    routed = tuple(backend.fused_jacobian_orders)
    assert set(routed) <= {1, 2, 3}
    u = field((9, 5, 67), 5, torch.float32)
    ud = u.to(DEV)
    calls = fused_calls(monkeypatch)
    for order in (1, 2, 3):
        fused = order in routed
        before = dict(calls)
        assert ops.jacobian_covered(ud, [order]) == fused
        v = ud.clone().requires_grad_()
        d = interpol.jacdet(v, interpolation=order, bound="dct2")
        J = interpol.jacobian(ud, interpolation=order, bound="dct2")
        torch.autograd.grad(d.sum(), v)
        assert (calls["fwd"] - before["fwd"], calls["field"] - before["field"]) == ((2, 1) if fused else (0, 0)), order
        assert_close(J, oracle_jacobian(u, 3, order), 1e-5, ("default routing", order))
        assert_close(d, oracle_det(u, 3, order), 1e-5, ("default routing", order))


@pytest.mark.parametrize("what", ["order0", "order5", "mixed", "bf16"])
def test_uncovered_classes_take_the_composed_route(what, monkeypatch):
    dtype = torch.bfloat16 if what == "bf16" else torch.float32
    u = field((9, 5, 67), 7, dtype)
    order = dict(order0=0, order5=5, mixed=[1, 2, 3], bf16=1)[what]
    ud = u.to(DEV)
    calls = fused_calls(monkeypatch)
    assert not ops.jacobian_covered(ud, order if isinstance(order, list) else [order])
    J = interpol.jacobian(ud, interpolation=order, bound="dct2")
    d = interpol.jacdet(ud, interpolation=order, bound="dct2")
    assert calls["fwd"] == 0 and J.dtype == dtype and d.dtype == dtype
    # (16-bit: the oracle sees the rounded values, in float32)
    assert_close(J.float(), oracle_jacobian(u.float(), 3, order), TOL[dtype], what)
    assert_close(d.float(), oracle_det(u.float(), 3, order), TOL[dtype], what)


# ---------------------------------------------------------------------------------------------------------------------
# 5. memory contract
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("misalign", [0, 1, 2, 3])
def test_memory_contract(misalign, dtype):
    for shape in ((9, 5, 67), (1, 2, 3), (19, 11), (130,), (2, 1, 1)):
        dim = len(shape)
        u = field(shape, 300 + dim, dtype)
        gout = torch.randn(u.shape[:-1], generator=torch.Generator().manual_seed(dim), dtype=torch.float64).to(dtype)
        ud, gd = u.to(DEV), gout.to(DEV)
        for order, bound in STENCILS:
            b, o = [bound] * dim, [order] * dim
            ref = (_hip.jacobian(ud, b, o), _hip.jacobian(ud, b, o, det_only=True), _hip.jacdet_backward_field(gd, ud, b, o))
            assert all(bool(torch.isfinite(r).all()) for r in ref)
            with memguard.installed(_hip, misalign=misalign) as seam:
                up, gp = memguard.place(u, DEV, misalign=misalign), memguard.place(gout, DEV, misalign=misalign)
                out = (_hip.jacobian(up, b, o), _hip.jacobian(up, b, o, det_only=True), _hip.jacdet_backward_field(gp, up, b, o))
                torch.cuda.synchronize()
                what = (shape, order, bound, misalign)
                assert len(seam.outputs()) == 3 and not seam.workspaces(), what
                assert out[1].shape == gout.shape and out[0].shape == (*u.shape, dim) and out[2].shape == (u.shape[0], dim, *u.shape[1:]), what
                off = misalign * u.element_size()
                assert out[0].data_ptr() % memguard.ALIGN == off and up.data_ptr() % memguard.ALIGN == off, what
                for t, r in zip(out, ref):
                    seam.assert_fully_written(t, r, what)
                    # no NaN from a read outside the field, and the very same values as from ordinary buffers
                    assert torch.equal(t, r), what
                seam.assert_guards_intact(what)
                for t in (up, gp):
                    memguard.assert_guard_intact(t, what)
                assert torch.equal(up, ud) and torch.equal(gp, gd), what


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_views_with_an_offset_and_strided_fields(dim):
    shape = {1: (130,), 2: (19, 11), 3: (9, 5, 67)}[dim]
    u = field(shape, 400 + dim, torch.float32).to(DEV)
    gout = torch.randn(u.shape[:-1], generator=torch.Generator().manual_seed(dim)).to(DEV)
    for order in (1, 3):
        b, o = [3] * dim, [order] * dim
        ref = (_hip.jacobian(u, b, o), _hip.jacobian(u, b, o, det_only=True), _hip.jacdet_backward_field(gout, u, b, o))
        # a view whose storage starts one element into its buffer
        buf = torch.full([u.numel() + 1], float("nan"), device=DEV)
        view = buf[1:].view(u.shape)
        view.copy_(u)
        assert view.storage_offset() == 1 and view.data_ptr() % 8 != 0
        # a field stored channel-first (not point by point), and every other item of a larger batch: made dense by the host
        chan = u.movedim(-1, 1).contiguous().movedim(1, -1)
        assert dim == 1 or not chan.is_contiguous()
        wide = torch.stack([u, u + 1], 1)[:, 0]
        assert wide.stride(0) == 2 * u.stride(0)
        for v in (view, chan, wide):
            got = (_hip.jacobian(v, b, o), _hip.jacobian(v, b, o, det_only=True), _hip.jacdet_backward_field(gout, v, b, o))
            for t, r in zip(got, ref):
                assert torch.equal(t, r), (dim, order)
            assert torch.equal(interpol.jacdet(v, interpolation=order, bound="dct2"), ref[1])
        # a gradient that is an expanded scalar
        g1 = torch.ones([], device=DEV).expand(gout.shape)
        assert torch.equal(_hip.jacdet_backward_field(g1, u, b, o), _hip.jacdet_backward_field(torch.ones_like(gout), u, b, o))
    with pytest.raises(ValueError):
        _hip.jacobian(u, [3] * dim, [1] * dim, out=u.view(-1)[:u.numel() // dim].view(u.shape[:-1]), det_only=True)   # the output inside the field


def test_entry_points_validate_before_launching():
    L = _hip.lib()
    shp = (6, 5, 4)
    f = torch.randn(1, *shp, 3, device=DEV)
    g = torch.randn(1, *shp, device=DEV)
    sentinel = 4321.0
    out = torch.full([1, *shp, 3, 3], sentinel, device=DEV)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    null = ctypes.c_void_p(0)

    def problem(order=(1, 1, 1), dtype=torch.float32, dstr=None, C=3, dim=3):
        st = [f.stride(0), 1, *f.stride()[1:4]]
        return _hip.make_problem(dim, dtype, dtype, [3] * 3, list(order), 1, 1, C, shp, shp, dstr or st, [0] * 5, [out.stride(0)] + [0] * 6, 0)

    def both(p):
        return (L.interpol_jacobian(ctypes.byref(p), ptr(f), ptr(out), 0, 1, null),
                L.interpol_jacdet_backward_field(ctypes.byref(p), ptr(g), ptr(f), ptr(out), null))

    assert both(problem(order=(0, 0, 0))) == (-2, -2)                   # INTERPOL_E_ORDER
    assert both(problem(order=(5, 5, 5))) == (-2, -2)
    assert both(problem(order=(1, 2, 3))) == (-2, -2)
    assert both(problem(dtype=torch.bfloat16)) == (-4, -4)              # INTERPOL_E_DTYPE
    assert both(problem(dstr=[f.stride(0), 120, 20, 4, 1])) == (-10, -10)     # a channel-first field: INTERPOL_E_STRIDE
    assert both(problem(C=2)) == (-5, -5)                               # components != dims: INTERPOL_E_SHAPE
    assert L.interpol_jacobian(ctypes.byref(problem()), null, ptr(out), 0, 1, null) == -6
    assert L.interpol_jacdet_backward_field(ctypes.byref(problem()), null, ptr(f), ptr(out), null) == -6
    torch.cuda.synchronize()
    assert bool((out == sentinel).all())
    assert both(problem()) == (0, 0)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and not bool((out == sentinel).any())


# ---------------------------------------------------------------------------------------------------------------------
# 6. determinism
# ---------------------------------------------------------------------------------------------------------------------
def test_two_identical_calls_give_identical_bits():
    for case, shape in enumerate(SHAPES):
        for dtype in (torch.float32, torch.float64):
            ud = field(shape, 500 + case, dtype).to(DEV)
            for order, bound in STENCILS:
                kw = dict(interpolation=order, bound=BOUNDS[bound])
                assert torch.equal(interpol.jacobian(ud, **kw), interpol.jacobian(ud, **kw))
                assert torch.equal(interpol.jacdet(ud, **kw), interpol.jacdet(ud, **kw))


# ---------------------------------------------------------------------------------------------------------------------
# 7. linear precision
# ---------------------------------------------------------------------------------------------------------------------
def linear_field(shape, seed, identity=False):
    """u(x) = (A - I) x + t with a random well-conditioned A -> (u (1,*shape,D), A), float64 on the CPU.  The entries of A and t
    are multiples of 1/64, so that u is exact in float32 as well: the test sees the kernel's error, not the rounding of its input."""
    dim = len(shape)
    gen = torch.Generator().manual_seed(seed)
    A = torch.eye(dim, dtype=torch.float64)
    if not identity:
        A = A + torch.randint(-16, 17, [dim, dim], generator=gen).double() / 64              # (diagonally dominant for D <= 3)
    t = torch.randint(-128, 129, [dim], generator=gen).double() / 64
    x = interpol.identity_grid(shape, dtype=torch.float64)
    return (x @ (A - torch.eye(dim, dtype=torch.float64)).T + t)[None], A


def inner(t, dim, margin=2):
    for d in range(dim):
        t = t.narrow(1 + d, margin, t.shape[1 + d] - 2 * margin)
    return t


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", [(130,), (19, 11), (9, 6, 67)], ids=["1d", "2d", "3d"])
def test_linear_precision(shape, dtype, monkeypatch):
    dim = len(shape)
    u, A = linear_field(shape, 70 + dim)
    ud = u.to(dtype).to(DEV)
    assert torch.equal(ud.cpu().double(), u)
    eye = torch.eye(dim, dtype=torch.float64)
    calls = fused_calls(monkeypatch)
    for order in (1, 2, 3):
        for bound in ("dct2", "zero", "dft"):
            J = inner(interpol.jacobian(ud, interpolation=order, bound=bound), dim)
            d = inner(interpol.jacdet(ud, interpolation=order, bound=bound), dim)
            assert J.numel() > 0
            assert_close(J, A.expand(J.shape), TOL[dtype], (shape, order, bound))
            assert_close(d, torch.linalg.det(A).expand(d.shape), TOL[dtype], ("det", shape, order, bound))
        # a translation under a periodic bound: the identity everywhere
        t, _ = linear_field(shape, 80 + dim, identity=True)
        td = t.to(dtype).to(DEV)
        J = interpol.jacobian(td, interpolation=order, bound="dft")
        assert_close(J, eye.expand(J.shape), TOL[dtype], ("translation", shape, order))
        d = interpol.jacdet(td, interpolation=order, bound="dft")
        assert_close(d, torch.ones(d.shape, dtype=torch.float64), TOL[dtype], ("translation det", shape, order))
    assert calls["fwd"] == 3 * 8
