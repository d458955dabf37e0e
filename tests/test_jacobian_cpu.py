"""`interpol.jacobian` / `interpol.jacdet` without a GPU: CPU tensors and 4-D fields run the composed form

    grid_grad(u.movedim(-1, 1), zeros, displacement=True, extrapolate=True).movedim(1, -2) + eye(D)

over the package's PyTorch kernel table.  The definition is the reference's `grid_grad(u channel-first, identity_grid(shape))`
plus the identity: its float64 answer is read from tests/golden/golden_jacobian.npz (recorded by
tests/golden/make_golden_jacobian.py from the live reference, which does not travel), and the C oracle restates it for
every order, bound and shape.

Fields are plain randn: the coordinates are the lattice points, exact in every dtype.
Bar: |got - want| <= tol |want| + tol max|want|, tol = 1e-11 (float64), 1e-5 (float32), 1e-2 (bf16 storage).
"""
import os

import numpy as np
import pytest
import torch

import interpol
from interpol import _hip, backend, ops
from interpol.torch_kernels import TorchKernels, cofactor_closed, det_closed
from oracle import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
BOUNDS = ["zero", "replicate", "dct1", "dct2", "dst1", "dst2", "dft"]
# the shapes the fused kernels are held to on the device (several workgroups of 256 points with a ragged last one; extents 1 / 2 / 3,
# where the stencil is wider than the volume and taps fold onto each other): the CPU route is held to the same ones
SHAPES = [(130,), (19, 11), (9, 5, 67), (3, 3, 3), (1, 2, 3), (2, 1, 1)]


def field(shape, seed, dtype=torch.float64, B=2):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn([B, *shape, len(shape)], generator=gen, dtype=torch.float64).to(dtype)


def within(got, want, tol):
    got, want = got.double(), want.double()
    err = (got - want).abs()
    allow = tol * want.abs() + tol * float(want.abs().max())
    return bool(torch.isfinite(got).all()) and bool((err <= allow).all()), float((err / allow.clamp_min(1e-300)).max())


def oracle_jacobian(u, bound, order):
    """oracle.grid_grad(u channel-first, identity_grid) + identity in the dtype of u; bound: one code or a per-dim list"""
    dim = u.shape[-1]
    shape = u.shape[1:-1]
    grid = interpol.identity_grid(shape, dtype=u.dtype)[None].expand(u.shape[0], *shape, dim).contiguous()
    bound = bound if isinstance(bound, list) else [bound] * dim
    g = torch.as_tensor(oracle.grid_grad(u.movedim(-1, 1).contiguous(), grid, bound, order, 1))
    return g.movedim(1, -2) + torch.eye(dim, dtype=u.dtype)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the recorded reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_jacobian_agrees_with_the_recorded_reference(dim):
    z = np.load(os.path.join(HERE, "golden", "golden_jacobian.npz"))
    u = torch.as_tensor(z["d%d_u" % dim]).double()
    eye = torch.eye(dim, dtype=torch.float64)
    k = 0
    while "d%d_c%d_want" % (dim, k) in z.files:
        order, bound = (int(v) for v in z["d%d_c%d_case" % (dim, k)])
        want = torch.as_tensor(z["d%d_c%d_want" % (dim, k)])
        kw = dict(interpolation=order, bound=BOUNDS[bound])
        got = interpol.jacobian(u, add_identity=False, **kw)
        assert got.shape == want.shape
        assert within(got, want, 1e-11)[0], (dim, order, bound)
        assert within(interpol.jacobian(u, **kw), want + eye, 1e-11)[0], (dim, order, bound)
        assert within(interpol.jacdet(u, **kw), torch.linalg.det(want + eye), 1e-11)[0], (dim, order, bound)
        k += 1
    assert k >= 4


# ---------------------------------------------------------------------------------------------------------------------
# 2. the C oracle, every order and bound
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_jacobian_matches_the_oracle_at_the_identity_grid(shape):
    u = field(shape, 10 + len(shape) + shape[0], B=1 if len(shape) == 3 else 2)
    for order in range(8):
        for bound in range(7):
            assert not ops.jacobian_covered(u, [order])
            want = oracle_jacobian(u, bound, order)
            kw = dict(interpolation=order, bound=BOUNDS[bound])
            ok, worst = within(interpol.jacobian(u, **kw), want, 1e-11)
            assert ok, (shape, order, bound, worst)
            ok, worst = within(interpol.jacdet(u, **kw), det_closed(want), 1e-11)
            assert ok, ("det", shape, order, bound, worst)


def test_jacobian_of_a_4d_field():
    shape = (3, 4, 2, 3)
    u = field(shape, 44)
    grid = interpol.identity_grid(shape, dtype=torch.float64)[None]
    for order, bound in ((1, 6), (3, 3), (2, 4)):
        want = TorchKernels.grad(u.movedim(-1, 1), grid, [bound] * 4, [order] * 4, 1).movedim(1, -2) + torch.eye(4, dtype=torch.float64)
        kw = dict(interpolation=order, bound=BOUNDS[bound])
        assert not ops.jacobian_covered(u, [order])
        assert within(interpol.jacobian(u, **kw), want, 1e-11)[0]
        assert within(interpol.jacdet(u, **kw), torch.linalg.det(want), 1e-11)[0]


def test_the_documented_differences():
    u = field((6, 7), 5)
    J = interpol.jacobian(u, interpolation=1, bound="dft", add_identity=False)
    for e in range(2):
        assert torch.equal(J[..., :, e], u.roll(-1, 1 + e) - u)                              # order 1: the FORWARD difference
    for order, side in ((2, 0.125), (3, 1.0 / 6.0)):
        J = interpol.jacobian(u, interpolation=order, bound="dft", add_identity=False)
        for e in range(2):
            o = 1 - e
            central = 0.5 * (u.roll(-1, 1 + e) - u.roll(1, 1 + e))
            smooth = side * (central.roll(-1, 1 + o) + central.roll(1, 1 + o)) + (1 - 2 * side) * central
            assert float((J[..., :, e] - smooth).abs().max()) <= 1e-14


# ---------------------------------------------------------------------------------------------------------------------
# 3. linear precision
# ---------------------------------------------------------------------------------------------------------------------
def linear_field(shape, seed, dtype=torch.float64, identity=False):
    """u(x) = (A - I) x + t with a random well-conditioned A -> (u (1,*shape,D), A)"""
    dim = len(shape)
    gen = torch.Generator().manual_seed(seed)
    A = torch.eye(dim, dtype=torch.float64)
    if not identity:
        A = A + 0.25 * (2 * torch.rand([dim, dim], generator=gen, dtype=torch.float64) - 1)   # (diagonally dominant for D <= 3)
    t = torch.randn([dim], generator=gen, dtype=torch.float64)
    x = interpol.identity_grid(shape, dtype=torch.float64)
    u = x @ (A - torch.eye(dim, dtype=torch.float64)).T + t
    return u[None].to(dtype), A


def inner(t, dim, margin=2):
    """the points at distance >= margin from all faces; t (1,*shape,...)"""
    for d in range(dim):
        t = t.narrow(1 + d, margin, t.shape[1 + d] - 2 * margin)
    return t


@pytest.mark.parametrize("shape", [(9,), (7, 8), (6, 7, 5)], ids=["1d", "2d", "3d"])
def test_linear_precision(shape):
    dim = len(shape)
    u, A = linear_field(shape, 70 + dim)
    for order in (1, 2, 3):
        for bound in ("dct2", "zero", "dft"):
            J = inner(interpol.jacobian(u, interpolation=order, bound=bound), dim)
            d = inner(interpol.jacdet(u, interpolation=order, bound=bound), dim)
            assert J.numel() > 0
            assert within(J, A.expand_as(J), 1e-11)[0], (shape, order, bound)
            assert within(d, torch.linalg.det(A).expand_as(d), 1e-11)[0], (shape, order, bound)
        # a translation under a periodic bound: the identity everywhere
        t, _ = linear_field(shape, 80 + dim, identity=True)
        J = interpol.jacobian(t, interpolation=order, bound="dft")
        assert within(J, torch.eye(dim, dtype=torch.float64).expand_as(J), 1e-11)[0]
        assert within(interpol.jacdet(t, interpolation=order, bound="dft"), torch.ones(t.shape[:-1], dtype=torch.float64), 1e-11)[0]


# ---------------------------------------------------------------------------------------------------------------------
# 4. / 5. gradients
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5,), (3, 2), (1, 2, 3), (2, 1, 1)], ids=lambda s: "x".join(map(str, s)))
def test_gradcheck_and_gradgradcheck(shape):
    u = field(shape, 90 + len(shape), B=1).requires_grad_()
    for order, bound in ((1, "dft"), (2, "dst1"), (3, "dct2")):
        kw = dict(interpolation=order, bound=bound)
        assert torch.autograd.gradcheck(lambda v: interpol.jacdet(v, **kw), (u,))
        assert torch.autograd.gradgradcheck(lambda v: interpol.jacdet(v, **kw), (u,))
        assert torch.autograd.gradcheck(lambda v: interpol.jacobian(v, **kw), (u,))
        assert torch.autograd.gradgradcheck(lambda v: interpol.jacobian(v, **kw), (u,))


def composed_jacobian(u, **kw):
    """through the public grid_grad, as a user without this feature writes it"""
    dim = u.shape[-1]
    return interpol.grid_grad(u.movedim(-1, 1), torch.zeros_like(u), displacement=True, extrapolate=True, **kw).movedim(1, -2) \
        + torch.eye(dim, dtype=u.dtype)


@pytest.mark.parametrize("shape", [(130,), (19, 11), (5, 4, 6), (1, 2, 3)], ids=lambda s: "x".join(map(str, s)))
def test_jacdet_backward_is_autograd_through_the_determinant(shape):
    u0 = field(shape, 95 + len(shape))
    w = torch.randn(u0.shape[:-1], generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    for order in (1, 2, 3):
        for bound in ("dft", "dct2", "zero", "dst1", "replicate"):
            kw = dict(interpolation=order, bound=bound)
            u = u0.clone().requires_grad_()
            got, = torch.autograd.grad((interpol.jacdet(u, **kw) * w).sum(), u)
            v = u0.clone().requires_grad_()
            want, = torch.autograd.grad((torch.linalg.det(composed_jacobian(v, **kw)) * w).sum(), v)
            assert float((got - want).abs().max()) <= 1e-11 * float(want.abs().max()), (shape, order, bound)
            # ... and the gradient of the matrix itself
            W = torch.randn([*u0.shape, u0.shape[-1]], generator=torch.Generator().manual_seed(3), dtype=torch.float64)
            got, = torch.autograd.grad((interpol.jacobian(u, **kw) * W).sum(), u)
            want, = torch.autograd.grad((composed_jacobian(v, **kw) * W).sum(), v)
            assert float((got - want).abs().max()) <= 1e-11 * float(want.abs().max()), (shape, order, bound)


def test_closed_forms():
    gen = torch.Generator().manual_seed(6)
    for D in (1, 2, 3, 4):
        J = torch.randn([5, D, D], generator=gen, dtype=torch.float64).requires_grad_()
        assert float((det_closed(J) - torch.linalg.det(J)).detach().abs().max()) <= 1e-13
        want, = torch.autograd.grad(torch.linalg.det(J).sum(), J)
        assert float((cofactor_closed(J) - want).detach().abs().max()) <= 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# 6. API contract
# ---------------------------------------------------------------------------------------------------------------------
def test_batches_fold_and_broadcast():
    u = field((6, 5), 12, B=3)
    J = interpol.jacobian(u)
    assert J.shape == (3, 6, 5, 2, 2) and interpol.jacdet(u).shape == (3, 6, 5)
    assert torch.equal(interpol.jacobian(u[0]), J[0]) and torch.equal(interpol.jacdet(u[0]), interpol.jacdet(u)[0])       # no batch
    assert torch.equal(interpol.jacobian(u[:1]), J[:1])                                                                   # a batch of 1
    stacked = u.reshape(3, 1, 6, 5, 2).expand(3, 2, 6, 5, 2)
    got = interpol.jacobian(stacked)
    assert got.shape == (3, 2, 6, 5, 2, 2) and torch.equal(got[:, 1], J)
    assert interpol.jacdet(stacked).shape == (3, 2, 6, 5)
    # defaults: linear, dft, identity added
    assert torch.equal(J, interpol.jacobian(u, interpolation=1, bound="dft", add_identity=True))
    assert torch.equal(J, interpol.jacobian(u, add_identity=False) + torch.eye(2, dtype=u.dtype))


def test_per_dim_lists():
    u = field((5, 4, 6), 13)
    kw = dict(interpolation=[1, 2, 3], bound=["dct2", "dft", "zero"])
    want = oracle_jacobian(u, [3, 6, 0], [1, 2, 3])
    assert within(interpol.jacobian(u, **kw), want, 1e-11)[0]
    assert within(interpol.jacdet(u, **kw), det_closed(want), 1e-11)[0]


def test_sixteen_bit_fields_compute_in_float32_and_round_once():
    u = field((9, 8, 7), 14, dtype=torch.bfloat16)
    for f in (interpol.jacobian, interpol.jacdet):
        got = f(u, interpolation=3, bound="dct2")
        want = f(u.float(), interpolation=3, bound="dct2")
        assert got.dtype == torch.bfloat16 and torch.equal(got, want.to(torch.bfloat16))
    v = u.clone().requires_grad_()
    g, = torch.autograd.grad(interpol.jacdet(v, interpolation=3, bound="dct2").float().sum(), v)
    assert g.dtype == torch.bfloat16 and g.shape == u.shape


def test_bad_fields_are_refused():
    with pytest.raises(ValueError):
        interpol.jacobian(torch.zeros(5, 6, 3))                          # last dim 3, two spatial dims
    with pytest.raises(ValueError):
        interpol.jacdet(torch.zeros(5, 6, 3))
    with pytest.raises(ValueError):
        interpol.jacobian(torch.zeros(5, 6, 0))                          # D = 0
    with pytest.raises(ValueError):
        interpol.jacobian(torch.zeros(2, 5, 6, 2).long())
    with pytest.raises(ValueError):
        interpol.jacdet(torch.zeros(2, 5, 6, 2, dtype=torch.int32))


# ---------------------------------------------------------------------------------------------------------------------
# 7. host logic with a fake library
# ---------------------------------------------------------------------------------------------------------------------
class FakeLibrary:
    """stands in for the three device calls of interpol/_hip.py on CPU tensors, and counts them"""

    def __init__(self):
        self.calls = dict(jacobian=0, jacdet=0, field=0)

    @staticmethod
    def covered(disp, order):
        order = [int(o) for o in list(order)[:disp.shape[-1]]]
        return disp.shape[-1] <= 3 and disp.dtype in (torch.float32, torch.float64) and len(set(order)) == 1 and 1 <= order[0] <= 3

    def jacobian(self, disp, bound, order, det_only=False, add_identity=True, out=None):
        self.calls["jacdet" if det_only else "jacobian"] += 1
        return TorchKernels.jacdet(disp, bound, order) if det_only else TorchKernels.jacobian(disp, bound, order, add_identity)

    def field(self, gout, disp, bound, order):
        self.calls["field"] += 1
        return (gout[..., None, None] * cofactor_closed(TorchKernels.jacobian(disp, bound, order))).movedim(-2, 1).contiguous()


@pytest.fixture
def fake(monkeypatch):
    lib = FakeLibrary()
    monkeypatch.setattr(_hip, "jacobian_covered", lib.covered)
    monkeypatch.setattr(_hip, "jacobian", lib.jacobian)
    monkeypatch.setattr(_hip, "jacdet_backward_field", lib.field)
    monkeypatch.setattr(ops._HipKernels, "grad", staticmethod(TorchKernels.grad))
    monkeypatch.setattr(ops._HipKernels, "pushgrad", staticmethod(TorchKernels.pushgrad))
    return lib


def test_routing_follows_fused_jacobian_orders(fake, monkeypatch):
    u = field((5, 4, 6), 15)
    table = type("Table", (ops._HipKernels,), {})                        # (a CPU tensor would get the PyTorch table otherwise)
    for routed in ((1, 2, 3), (1,), ()):
        monkeypatch.setattr(backend, "fused_jacobian_orders", routed)
        for order in (0, 1, 2, 3, 5):
            assert ops._HipKernels.jacobian_fused(u, [order] * 3) == (order in routed)
            before = dict(fake.calls)
            with ops.use_kernels(table):
                v = u.clone().requires_grad_()
                J = interpol.jacobian(v, interpolation=order, bound="dct2")
                d = interpol.jacdet(v, interpolation=order, bound="dct2")
                g, = torch.autograd.grad(d.sum(), v)
            new = {k: fake.calls[k] - before[k] for k in before}
            assert new == ({"jacobian": 1, "jacdet": 1, "field": 1} if order in routed else {"jacobian": 0, "jacdet": 0, "field": 0}), (routed, order)
            # either route: the same values
            w = u.clone().requires_grad_()
            assert torch.equal(J, interpol.jacobian(w, interpolation=order, bound="dct2"))
            dw = interpol.jacdet(w, interpolation=order, bound="dct2")
            assert torch.equal(d, dw)
            gw, = torch.autograd.grad(dw.sum(), w)
            assert float((g - gw).abs().max()) <= 1e-12 * max(1.0, float(gw.abs().max()))


def test_uncovered_classes_take_the_composed_route(fake):
    table = type("Table", (ops._HipKernels,), {})
    cases = [(field((5, 4, 6), 16), [1, 2, 3]), (field((5, 4, 6), 16), 0), (field((5, 4, 6), 16), 4),
             (field((5, 4, 6), 16, dtype=torch.bfloat16), 1)]
    for u, order in cases:
        assert not ops._HipKernels.jacobian_fused(u, order if isinstance(order, list) else [order] * 3)
        with ops.use_kernels(table):
            J = interpol.jacobian(u, interpolation=order, bound="dft")
            d = interpol.jacdet(u, interpolation=order, bound="dft")
        assert J.dtype == u.dtype and d.dtype == u.dtype
        assert torch.equal(J, interpol.jacobian(u, interpolation=order, bound="dft"))
        assert torch.equal(d, interpol.jacdet(u, interpolation=order, bound="dft"))
    assert fake.calls == dict(jacobian=0, jacdet=0, field=0)
    # a CPU tensor is never covered, whatever the order
    assert not ops.jacobian_covered(field((5, 4), 1), [1])
