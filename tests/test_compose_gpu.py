"""`interpol.compose` / `interpol.exp` on the device (csrc/compose.hip).

Definition everywhere: compose(left, right) = right + grid_pull(left channel-first, right, displacement=True) moved back to
(..., D).  Forward truth: the C oracle in the field's dtype; backward truth: the float64 composed route on the device,
differentiated by autograd through the existing operators -- never the code under test.

Inputs of every parity test: displacements are multiples of 1/64 with |.| <= 6 on lattices of edge <= 64, so every
coordinate o + right is exact in float32 and float64 alike -- both precisions see the same `floor` and the same
extrapolation mask (tests/test_affine_grad_gpu.py uses the same device); `left` is unrestricted randn.

Bars.  Forward: |got - want| <= tol |want| + tol max|pulled term of want|, tol = 1e-5 (float32) / 1e-11 (float64) /
1e-2 (bf16 storage).  Backward: rtol = tol, atol = tol max|ref| per gradient.

Routing: the library instantiates orders 1, 2 and 3; `interpol.backend.fused_compose_orders` (default: order 1, the order at
which the fused kernel was measured faster) decides which of them the host layer sends there.  The tests below run with
all three routed to the fused kernels, so that every instantiation is held to the bars; one test checks the default.

memguard's `misalign` counts ELEMENTS (0..3): one element is the 4 bytes (float32) / 8 bytes (float64) that take a
D-component point off 12- / 16- / 24-byte alignment.
"""
import numpy as np
import pytest
import torch

import interpol
from interpol import _hip, backend, ops
from oracle import oracle
import memguard

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = {torch.float32: 1e-5, torch.float64: 1e-11, torch.bfloat16: 1e-2}
BOUNDS = ["zero", "replicate", "dct1", "dct2", "dst1", "dst2", "dft"]
# (lshape, oshape): the smallest that can still break the kernel; the last: 51 800 samples, a ragged final block
SHAPES = [((67,), (130,)), ((13, 22), (19, 11)), ((13, 10, 17), (11, 14, 9)), ((37, 40, 35), (37, 40, 35))]
SMALL = {1: SHAPES[0], 2: SHAPES[1], 3: SHAPES[2]}
# (order, bound code): all seven bounds for order 1; dct2, dft, zero, dst1 for orders 2 - 3
STENCILS = [(1, b) for b in range(7)] + [(k, b) for k in (2, 3) for b in (3, 6, 0, 4)]


@pytest.fixture(autouse=True)
def every_instantiated_order_fused(monkeypatch):
    monkeypatch.setattr(backend, "fused_compose_orders", (1, 2, 3))


def dyadic(gen, shape, amp=6, dtype=torch.float32):
    return torch.randint(-64 * amp, 64 * amp + 1, shape, generator=gen).to(dtype) / 64


def fields(lshape, oshape, seed, dtype, B=2):
    gen = torch.Generator().manual_seed(seed)
    dim = len(oshape)
    left = torch.randn([B, *lshape, dim], generator=gen).to(dtype)
    right = dyadic(gen, [B, *oshape, dim]).to(dtype)
    return left, right


def oracle_compose(left, right, bound, order, ex):
    """right + oracle.grid_pull(left channel-first, add_identity_grid(right)) in the fields' dtype (CPU tensors);
    -> (want, max |pulled term|) in float64"""
    dim = right.shape[-1]
    grid = interpol.add_identity_grid(right)
    pulled = torch.as_tensor(oracle.grid_pull(left.movedim(-1, 1).contiguous(), grid, [bound] * dim, order, ex)).movedim(1, -1)
    return (right + pulled).double(), float(pulled.double().abs().max())


def assert_forward(got, want, pulled_max, tol, what):
    err = (got.detach().cpu().double() - want).abs()
    allow = tol * want.abs() + tol * pulled_max
    assert bool(torch.isfinite(got).all()), what
    assert bool((err <= allow).all()), (what, float((err / allow.clamp_min(1e-300)).max()))


def composed(left, right, **kw):
    dim = right.shape[-1]
    return right + interpol.grid_pull(left.movedim(-1, -dim - 1), right, displacement=True, **kw).movedim(-dim - 1, -1)


def fused_calls(monkeypatch):
    """count the calls that reach the two entry points of the library"""
    calls = dict(fwd=0, bwd=0)
    fwd, bwd = _hip.compose, _hip.compose_backward_right

    def f(*a, **k):
        calls["fwd"] += 1
        return fwd(*a, **k)

    def b(*a, **k):
        calls["bwd"] += 1
        return bwd(*a, **k)

    monkeypatch.setattr(_hip, "compose", f)
    monkeypatch.setattr(_hip, "compose_backward_right", b)
    return calls


# ---------------------------------------------------------------------------------------------------------------------
# 1. forward parity against the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", range(len(SHAPES)))
def test_compose_forward_matches_the_oracle(case, dtype, monkeypatch):
    lshape, oshape = SHAPES[case]
    left, right = fields(lshape, oshape, 100 + case, dtype)
    l, r = left.to(DEV), right.to(DEV)
    calls = fused_calls(monkeypatch)
    n = 0
    for order, bound in STENCILS:
        for ex in (0, 1, 2):
            assert ops.compose_covered(l, r, [order])
            got = interpol.compose(l, r, interpolation=order, bound=BOUNDS[bound], extrapolate=ex)
            assert got.shape == r.shape and got.dtype == dtype
            assert_forward(got, *oracle_compose(left, right, bound, order, ex), TOL[dtype], (lshape, order, bound, ex))
            n += 1
            if ex == 1:
                # left broadcast from a batch of 1
                got = interpol.compose(l[:1], r, interpolation=order, bound=BOUNDS[bound], extrapolate=ex)
                assert_forward(got, *oracle_compose(left[:1], right, bound, order, ex), TOL[dtype], ("broadcast", lshape, order, bound))
                n += 1
    assert calls["fwd"] == n            # every call went through interpol_compose


def test_compose_default_routing_sends_order_one_to_the_fused_kernel(monkeypatch):
    monkeypatch.undo()                                                   # (the package's own default)
    assert tuple(backend.fused_compose_orders) == (1,)
    lshape, oshape = SMALL[3]
    left, right = fields(lshape, oshape, 5, torch.float32)
    l, r = left.to(DEV), right.to(DEV)
    calls = fused_calls(monkeypatch)
    for order, fused in ((1, True), (2, False), (3, False)):
        before = calls["fwd"]
        assert ops.compose_covered(l, r, [order]) == fused
        got = interpol.compose(l, r, interpolation=order, bound="dct2", extrapolate=True)
        assert (calls["fwd"] - before == 1) == fused
        assert_forward(got, *oracle_compose(left, right, 3, order, 1), 1e-5, ("default routing", order))


@pytest.mark.parametrize("what", ["order0", "order5", "mixed", "bf16"])
def test_compose_uncovered_classes_take_the_composed_route(what, monkeypatch):
    lshape, oshape = SMALL[3]
    dtype = torch.bfloat16 if what == "bf16" else torch.float32
    left, right = fields(lshape, oshape, 7, dtype)
    order = dict(order0=0, order5=5, mixed=[1, 2, 3], bf16=1)[what]
    l, r = left.to(DEV), right.to(DEV)
    calls = fused_calls(monkeypatch)
    assert not ops.compose_covered(l, r, order if isinstance(order, list) else [order])
    got = interpol.compose(l, r, interpolation=order, bound="dct2", extrapolate=True)
    assert calls["fwd"] == 0 and got.dtype == dtype and got.shape == r.shape
    # (16-bit: the oracle sees the rounded values, in float32)
    want, pm = oracle_compose(left.float(), right.float(), 3, order, 1)
    assert_forward(got.float(), want, pm, TOL[dtype], what)


# ---------------------------------------------------------------------------------------------------------------------
# 2. backward parity against the float64 composed route on the device
# ---------------------------------------------------------------------------------------------------------------------
def _grads(f, left, right, w, **kw):
    l, r = left.clone().requires_grad_(), right.clone().requires_grad_()
    return torch.autograd.grad((f(l, r, **kw) * w).sum(), (l, r))


def assert_grad(got, ref, tol, what):
    err = (got.double() - ref).abs()
    allow = tol * ref.abs() + tol * float(ref.abs().max())
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), what
    assert bool((err <= allow).all()), (what, float((err / allow.clamp_min(1e-300)).max()))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_compose_backward_matches_the_composed_route(dim, dtype, monkeypatch):
    lshape, oshape = SMALL[dim]
    left, right = fields(lshape, oshape, 200 + dim, dtype)
    w = torch.randn(right.shape, generator=torch.Generator().manual_seed(dim)).to(dtype)
    l, r, wd = left.to(DEV), right.to(DEV), w.to(DEV)
    calls = fused_calls(monkeypatch)
    n = 0
    for order in (1, 3):
        for bound in ("dct2", "dft"):
            for ex in (1, 0):
                kw = dict(interpolation=order, bound=bound, extrapolate=ex)
                ref_l, ref_r = _grads(composed, l.double(), r.double(), wd.double(), **kw)
                got_l, got_r = _grads(interpol.compose, l, r, wd, **kw)
                n += 1
                assert_grad(got_r, ref_r, TOL[dtype], ("grad_right", dim, order, bound, ex))
                assert_grad(got_l, ref_l, TOL[dtype], ("grad_left", dim, order, bound, ex))
    assert calls["fwd"] == n and calls["bwd"] == n
    # a broadcast `left`: its gradient is summed over the batch
    kw = dict(interpolation=3, bound="dct2", extrapolate=1)
    ref_l, ref_r = _grads(composed, l[:1].double().expand_as(l), r.double(), wd.double(), **kw)
    got_l, got_r = _grads(interpol.compose, l[:1], r, wd, **kw)
    assert_grad(got_r, ref_r, TOL[dtype], "broadcast grad_right")
    assert_grad(got_l, ref_l.sum(0, keepdim=True), TOL[dtype], "broadcast grad_left")


def test_compose_double_backward_matches_the_composed_route():
    lshape, oshape = SMALL[2]
    left, right = fields(lshape, oshape, 31, torch.float64)
    kw = dict(interpolation=3, bound="dct2", extrapolate=True)
    res = []
    for f in (interpol.compose, composed):
        l, r = left.to(DEV).requires_grad_(), right.to(DEV).requires_grad_()
        g1, = torch.autograd.grad(f(l, r, **kw).square().sum(), r, create_graph=True)
        res.append(torch.autograd.grad(g1.square().sum(), (l, r)))
    for a, b in zip(*res):
        assert bool(torch.isfinite(a).all())
        assert float((a - b).abs().max()) <= 1e-9 * float(b.abs().max())


def test_compose_gradcheck_runs_the_fused_kernels(monkeypatch):
    gen = torch.Generator().manual_seed(17)
    left = torch.randn([1, 5, 6, 2], generator=gen, dtype=torch.float64).to(DEV).requires_grad_()
    right = (1.5 * torch.randn([1, 5, 6, 2], generator=gen, dtype=torch.float64)).to(DEV).requires_grad_()
    calls = fused_calls(monkeypatch)
    assert torch.autograd.gradcheck(lambda l, r: interpol.compose(l, r, interpolation=3, bound="dct2", extrapolate=True), (left, right))
    assert calls["fwd"] > 0 and calls["bwd"] > 0


# ---------------------------------------------------------------------------------------------------------------------
# 3. no channel-first intermediate
# ---------------------------------------------------------------------------------------------------------------------
def _rise(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return out, torch.cuda.max_memory_allocated() - base


def test_fused_forward_allocates_the_output_only():
    gen = torch.Generator().manual_seed(3)
    shape = [2, 64, 64, 96, 3]
    left = torch.randn(shape, generator=gen).to(DEV)
    right = dyadic(gen, shape, amp=2).to(DEV)
    nbytes = left.numel() * 4
    with torch.no_grad():
        interpol.compose(left[:, :8], right[:, :8])                      # (the library is loaded)
        out, rise = _rise(lambda: interpol.compose(left, right, interpolation=1))
        assert out.numel() * 4 == nbytes
        assert rise <= 1.25 * nbytes, (rise, nbytes)
        out2, rise = _rise(lambda: interpol.exp(right, steps=4))
        assert rise <= 2.25 * nbytes, (rise, nbytes)
        del out, out2
        # the composed route needs at least twice the output (the yardstick of the condition above)
        _, rise = _rise(lambda: composed(left, right, interpolation=1, bound="dft", extrapolate=True))
        assert rise >= 2 * nbytes


# ---------------------------------------------------------------------------------------------------------------------
# 4. memory contract
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", [(13, 10, 17), (1, 1, 3), (7, 1)], ids=["13x10x17", "1x1x3", "7x1"])
def test_compose_memory_contract(shape, dtype):
    dim = len(shape)
    gen = torch.Generator().manual_seed(len(shape) * 100 + shape[0])
    left = torch.randn([2, *shape, dim], generator=gen).to(dtype)
    right = dyadic(gen, [2, *shape, dim]).to(dtype)
    gout = torch.randn([2, *shape, dim], generator=gen).to(dtype)
    for order in (1, 2, 3):
        for bound in range(7):
            for ex in (1, 0):
                b, o = [bound] * dim, [order] * dim
                ref = _hip.compose(left.to(DEV), right.to(DEV), b, o, ex)
                ref_g = _hip.compose_backward_right(gout.to(DEV), left.to(DEV), right.to(DEV), b, o, ex)
                assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(ref_g).all())
                with memguard.installed(_hip, misalign=1) as seam:
                    l, r, g = (memguard.place(t, DEV, misalign=1) for t in (left, right, gout))
                    out = _hip.compose(l, r, b, o, ex)
                    gr = _hip.compose_backward_right(g, l, r, b, o, ex)
                    torch.cuda.synchronize()
                    what = (shape, order, bound, ex)
                    assert len(seam.outputs()) == 2 and not seam.workspaces(), what
                    assert out.data_ptr() % 16 != 0 and l.data_ptr() % 16 != 0
                    seam.assert_fully_written(out, ref, what)
                    seam.assert_fully_written(gr, ref_g, what)
                    seam.assert_guards_intact(what)
                    for t in (l, r, g):
                        memguard.assert_guard_intact(t, what)
                    # no NaN from a read outside `left`, and the very same values as from ordinary buffers
                    assert torch.equal(out, ref) and torch.equal(gr, ref_g), what
                    assert torch.equal(l, left.to(DEV)) and torch.equal(r, right.to(DEV)) and torch.equal(g, gout.to(DEV)), what


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_compose_output_may_alias_right(dim):
    lshape, oshape = SMALL[dim]
    left, right = fields(lshape, oshape, 300 + dim, torch.float32)
    l, r = left.to(DEV), right.to(DEV)
    for order in (1, 3):
        fresh = ops.compose(l, r, [3], [order], 1)
        buf = r.clone()
        res = ops.compose(l, buf, [3], [order], 1, out=buf)
        assert res.data_ptr() == buf.data_ptr() and torch.equal(res, fresh)
    with pytest.raises(ValueError):
        sq = r.clone()
        ops.compose(sq, sq, [3], [1], 1, out=sq)                        # the output must not be `left`


def test_compose_entry_points_validate_before_launching():
    import ctypes
    L = _hip.lib()
    shp = (6, 5, 4)
    f = torch.randn(1, *shp, 3, device=DEV)
    sentinel = 4321.0
    out = torch.full_like(f, sentinel)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    null = ctypes.c_void_p(0)

    def problem(order=(1, 1, 1), dtype=torch.float32, lstr=None, C=3):
        st = [f.stride(0), 1, *f.stride()[1:4]]
        return _hip.make_problem(3, dtype, dtype, [3] * 3, list(order), 1, 1, C, shp, shp, lstr or st,
                                 [f.stride(0), *f.stride()[1:4], 1], st + [0, 0], 0)

    def both(p):
        return (L.interpol_compose(ctypes.byref(p), ptr(f), ptr(f), ptr(out), null),
                L.interpol_compose_backward_right(ctypes.byref(p), ptr(f), ptr(f), ptr(f), ptr(out), null))

    assert both(problem(order=(0, 0, 0))) == (-2, -2)                   # INTERPOL_E_ORDER
    assert both(problem(order=(5, 5, 5))) == (-2, -2)
    assert both(problem(order=(1, 2, 3))) == (-2, -2)
    assert both(problem(dtype=torch.bfloat16)) == (-4, -4)              # INTERPOL_E_DTYPE
    assert both(problem(lstr=[f.stride(0), 120, 20, 4, 1])) == (-10, -10)     # a channel-first `left`: INTERPOL_E_STRIDE
    assert L.interpol_compose(ctypes.byref(problem()), null, ptr(f), ptr(out), null) == -6
    torch.cuda.synchronize()
    assert bool((out == sentinel).all())
    assert both(problem()) == (0, 0)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and not bool((out == sentinel).any())


# ---------------------------------------------------------------------------------------------------------------------
# 5. exp
# ---------------------------------------------------------------------------------------------------------------------
def test_exp_is_scaling_and_squaring():
    gen = torch.Generator().manual_seed(9)
    vel = dyadic(gen, [2, 11, 14, 9, 3], amp=2).to(DEV)
    with torch.no_grad():
        assert torch.equal(interpol.exp(vel, steps=0), vel)
        u = vel * 0.125
        for _ in range(3):
            u = interpol.compose(u, u)
        assert torch.equal(interpol.exp(vel, 3), u)
        assert torch.equal(interpol.exp(vel, 3, inverse=True), interpol.exp(-vel, 3))
    # with a graph: the same bits as without
    v = vel.clone().requires_grad_()
    assert torch.equal(interpol.exp(v, 3).detach(), u)


def _smooth_velocity(shape, amp, gen):
    """low-pass noise of amplitude `amp`: a few random Fourier modes per component"""
    dim = len(shape)
    axes = torch.meshgrid(*[torch.arange(n, dtype=torch.float64) / n for n in shape], indexing="ij")
    v = torch.zeros([*shape, dim], dtype=torch.float64)
    for d in range(dim):
        for _ in range(4):
            k = torch.randint(1, 3, [dim], generator=gen)
            ph = 2 * np.pi * float(torch.rand([], generator=gen))
            v[..., d] += torch.sin(2 * np.pi * sum(float(k[e]) * axes[e] for e in range(dim)) + ph)
    return v * (amp / float(v.abs().max()))


def test_exp_accuracy_and_gradient_against_the_float64_composed_route():
    gen = torch.Generator().manual_seed(12)
    shape = (24, 20, 28)
    vel = _smooth_velocity(shape, 2.0, gen)[None].to(DEV)
    w = torch.randn(vel.shape, generator=gen, dtype=torch.float64).to(DEV)
    kw = dict(interpolation=1, bound="dft", extrapolate=True)

    def exp_composed(v):
        u = v * 2.0 ** -4
        for _ in range(4):
            u = composed(u, u, **kw)
        return u

    def run(f, dtype):
        v = vel.to(dtype).requires_grad_()
        y = f(v)
        g, = torch.autograd.grad((y * w.to(dtype)).sum(), v)
        return y.detach().double(), g.double()

    ref_y, ref_g = run(exp_composed, torch.float64)
    yard_y, yard_g = run(exp_composed, torch.float32)
    got_y, got_g = run(lambda v: interpol.exp(v, 4, **kw), torch.float32)
    for name, got, yard, ref in (("exp", got_y, yard_y, ref_y), ("gradient", got_g, yard_g, ref_g)):
        e_got, e_yard = float((got - ref).abs().max()), float((yard - ref).abs().max())
        bar = max(1e-5 * float(ref.abs().max()), 2 * e_yard)
        print("exp steps=4 %s: fused float32 error %.3g, composed float32 error %.3g, bar %.3g" % (name, e_got, e_yard, bar))
        assert e_got <= bar, (name, e_got, e_yard, bar)


def test_exp_in_a_captured_graph():
    gen = torch.Generator().manual_seed(21)
    static = dyadic(gen, [1, 24, 20, 28, 3], amp=2).to(DEV)
    with torch.no_grad():
        interpol.exp(static, 2)                                          # (library loaded, allocator warm)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = interpol.exp(static, 2)
        for it in range(2):
            static.copy_(dyadic(gen, list(static.shape), amp=2))
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, interpol.exp(static, 2)), it
