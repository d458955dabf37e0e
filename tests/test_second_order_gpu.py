"""grid_hess, grid_pushgrad and grid_grad_backward on the device (csrc/ops_generic.hpp: hess_generic, pushgrad_generic): what every
double backward of pull, push, count and grid_grad reaches on CUDA tensors, and the backward of jacobian / jacdet.

Truth: the C oracle at extrapolate = 1 (pinned against the reference for every order and bound) and, under a mask, the identity
`masked_truth` of tests/test_second_order_cpu.py -- never the code under test, and never the reference, which raises for a masked
Hessian (SURVEY B-2).  Inputs, shapes and the form of the bar come from that module (see its docstring): coordinates are multiples
of 1/64, so float32 and float64 see the same `floor` and the same mask; 10 - 60 % of the samples are masked at ex = 0.

Bars: |got - want| <= tol |want| + tol max(max|want|, max|input values|); tol = 1e-5 float32 (golden_util.fp32_tol), 1e-11 float64
(the float64 goldens), 1e-2 / 2e-3 bf16 / f16 storage (test_low_precision_storage).

Shapes.  Both kernels run one thread per sample in blocks of 256, the batch over blockIdx.y: there is no tile to straddle.
(67,) <- (300,): two blocks, the last ragged; (13, 22) <- (19, 11) ends inside one block; (13, 10, 17) <- (11, 14, 9) is 1386
samples, six blocks, rows and planes inside a block; on (1,), (2,), (1, 4) and (2, 1, 3) an order-7 stencil wraps the extent
several times.
"""
import numpy as np
import pytest
import torch

import golden_util as G
import interpol
import memguard
from interpol import _hip, ops
from oracle import oracle
from oracle_kernels import OracleKernels
import test_second_order_cpu as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = {torch.float32: G.fp32_tol()[0], torch.float64: 1e-11, torch.bfloat16: 1e-2, torch.float16: 2e-3}
assert G.fp32_tol() == (1e-5, 1e-5)
DTYPES = [torch.float32, torch.float64]
IDS = ["f32", "f64"]
masked_truth, ratio, amax, problem = S.masked_truth, S.ratio, S.amax, S.problem
_TRUTH = {}


def _threads(fn):
    oracle.set_threads(8)
    try:
        return fn()
    finally:
        oracle.set_threads(1)


def truths(dim, case, order, bound):
    """{("hess" | "pushgrad", ex): numpy float64} of one (shape, stencil) for ex = 1, 0, 2: computed once, shared by the dtypes of a
    test and by the tests of one dim (the cache holds one dim at a time), never modified."""
    if _TRUTH.get("dim") != dim:
        _TRUTH.clear()
        _TRUTH["dim"] = dim
    key = (case, tuple(order), tuple(bound))
    if key not in _TRUTH:
        lattice, samples = S.SHAPES[dim][case]
        p = problem(lattice, samples)

        def make():
            base = np.asarray(oracle.grid_hess(p["inp"], p["grid"], bound, order, 1))
            r = {}
            for ex in (1, 0, 2):
                r["hess", ex] = base if ex == 1 else masked_truth("hess", p["inp"], p["grid"], bound, order, ex, base=base)
                r["pushgrad", ex] = (np.asarray(oracle.grid_pushgrad(p["val"], p["grid"], lattice, bound, order, 1)) if ex == 1 else
                                     masked_truth("pushgrad", p["val"], p["grid"], bound, order, ex, shape=lattice))
            return r
        _TRUTH[key] = _threads(make)
    return _TRUTH[key]


def on_device(p, dtype):
    return {k: (v.to(DEV, dtype) if torch.is_tensor(v) else v) for k, v in p.items()}


def hip_calls(monkeypatch):
    """count the calls that reach the two entry points of the host layer, by operator"""
    calls = {}
    gather, scatter = _hip.gather, _hip.scatter

    def g(op, *a, **k):
        calls[op] = calls.get(op, 0) + 1
        return gather(op, *a, **k)

    def s(op, *a, **k):
        calls[op] = calls.get(op, 0) + 1
        return scatter(op, *a, **k)

    monkeypatch.setattr(_hip, "gather", g)
    monkeypatch.setattr(_hip, "scatter", s)
    return calls


def _sweep(dim, dtype, stencils):
    """hess and pushgrad of every shape of `dim` through ops.*, all three extrapolation modes -> {(op, order): worst error / allowed}"""
    tol = TOL[dtype]
    worst = {}
    for case, (lattice, samples) in enumerate(S.SHAPES[dim]):
        p = problem(lattice, samples)
        d = on_device(p, dtype)
        fi, fv = amax(p["inp"]), amax(p["val"])
        for order, bound in stencils:
            want = truths(dim, case, order, bound)
            for ex in (1, 0, 2):
                got = ops.grid_hess(d["inp"], d["grid"], bound, order, ex)
                assert got.dtype == dtype and list(got.shape) == [S.B, S.C, *samples, dim, dim]
                rh = ratio(got, want["hess", ex], tol, fi)
                got = ops.grid_pushgrad(d["val"], d["grid"], lattice, bound, order, ex)
                assert got.dtype == dtype and list(got.shape) == [S.B, S.C, *lattice]
                rp = ratio(got, want["pushgrad", ex], tol, fv)
                k = "".join(map(str, order))
                worst["hess", k] = max(worst.get(("hess", k), 0.0), rh)
                worst["pushgrad", k] = max(worst.get(("pushgrad", k), 0.0), rp)
                assert rh <= 1.0 and rp <= 1.0, (lattice, samples, order, bound, ex, str(dtype), "hess %.3g pushgrad %.3g" % (rh, rp))
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# 1. every order x every bound x every extrapolation mode
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_hess_and_pushgrad_match_the_oracle(dim, dtype):
    worst = _sweep(dim, dtype, [([k], [b]) for k in range(8) for b in range(7)])
    for (op, k), r in sorted(worst.items()):
        print("second_order margin: op=%s dtype=%s dim=%d order=%s worst error / allowed = %.4f" % (op, str(dtype).split(".")[1], dim, k, r))


# ---------------------------------------------------------------------------------------------------------------------
# 2. one order and one bound per dim
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_mixed_orders_and_bounds(dim, dtype):
    worst = _sweep(dim, dtype, [(o, b) for o, b in S.MIXED])
    for (op, k), r in sorted(worst.items()):
        print("second_order mixed: op=%s dtype=%s dim=%d orders=%s worst error / allowed = %.4f" % (op, str(dtype).split(".")[1], dim, k, r))


# ---------------------------------------------------------------------------------------------------------------------
# 3. the forms an input can take
# ---------------------------------------------------------------------------------------------------------------------
FORMS = [([3], [3], 0), ([4], [6], 2), ([6], [4], 1), ([2, 3, 5], [2, 5, 0], 0)]


def _affine(lattice, samples, dtype):
    """a dyadic (D, D+1) matrix whose lattice overhangs `lattice` like problem()'s: scale on the diagonal, a shear of 1/64 per
    sample off it; every product with a sample index is exact, so AffineGrid.dense() has the very coordinates of the kernel"""
    dim = len(lattice)
    h = S.OVERHANG[dim]
    mat = torch.zeros(dim, dim + 1, dtype=torch.float64)
    for d in range(dim):
        mat[d, d] = round(64 * (lattice[d] - 1 + 2 * h) / max(samples[d] - 1, 1)) / 64
        for e in range(dim):
            if e != d:
                mat[d, e] = (1 + d + e) / 64
        mat[d, dim] = -h
    return mat.to(dtype)


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_input_forms(dim):
    lattice, samples = S.SHAPES[dim][0]
    p = problem(lattice, samples)
    gen = torch.Generator().manual_seed(77 + dim)
    for dtype in DTYPES:
        tol = TOL[dtype]
        d = on_device(p, dtype)
        inp, val, grid = d["inp"], d["val"], d["grid"]
        fi, fv = amax(p["inp"]), amax(p["val"])
        for order, bound, ex in FORMS:
            what = (dim, str(dtype), order, bound, ex)

            def check(got, want, floor, tag):
                r = ratio(got, want, tol, floor)
                assert r <= 1.0, what + (tag, r)

            want_h = _threads(lambda: masked_truth("hess", p["inp"], p["grid"], bound, order, ex))
            want_p = _threads(lambda: masked_truth("pushgrad", p["val"], p["grid"], bound, order, ex, shape=lattice))
            ref_h = ops.grid_hess(inp, grid, bound, order, ex)
            check(ref_h, want_h, fi, "hess")
            # displacement = True: the kernel adds the identity lattice of the samples
            disp = (p["grid"] - interpol.identity_grid(samples, dtype=torch.float64)).to(DEV, dtype)
            check(ops.grid_hess(inp, disp, bound, order, ex, displacement=True), want_h, fi, "hess displacement")
            check(ops.grid_pushgrad(val, disp, lattice, bound, order, ex, displacement=True), want_p, fv, "pushgrad displacement")
            # lazy lattices: against the oracle on their dense()
            lins = [S.dyadic_line(n, m, S.OVERHANG[dim]) + torch.randint(-64, 65, [m], generator=gen).double() / 64
                    for n, m in zip(lattice, samples)]
            for lazy in (interpol.SeparableGrid([l.to(dtype) for l in lins]), interpol.AffineGrid(_affine(lattice, samples, dtype), samples)):
                dense = lazy.dense().double()
                assert torch.equal(dense * 64, torch.round(dense * 64)) and S.masked_share(dense, lattice, 0) > 0.05
                name = type(lazy).__name__
                check(ops.grid_hess(inp, lazy.to(DEV), bound, order, ex),
                      _threads(lambda: masked_truth("hess", p["inp"], dense, bound, order, ex)), fi, "hess " + name)
                check(ops.grid_pushgrad(val, lazy.to(DEV), lattice, bound, order, ex),
                      _threads(lambda: masked_truth("pushgrad", p["val"], dense, bound, order, ex, shape=lattice)), fv, "pushgrad " + name)
                gi, gg = ops.grid_grad_backward(d["grad"], inp, lazy.to(DEV), bound, order, ex, need_inp=True, need_grid=False)
                assert gg is None
                check(gi, _threads(lambda: masked_truth("pushgrad", p["grad"], dense, bound, order, ex, shape=lattice)), amax(p["grad"]),
                      "grad_backward " + name)
            # batch broadcast, either way
            check(ops.grid_hess(inp[:1], grid, bound, order, ex),
                  _threads(lambda: masked_truth("hess", p["inp"][:1], p["grid"], bound, order, ex)), fi, "hess: inp of batch 1")
            check(ops.grid_hess(inp, grid[:1], bound, order, ex),
                  _threads(lambda: masked_truth("hess", p["inp"], p["grid"][:1], bound, order, ex)), fi, "hess: grid of batch 1")
            check(ops.grid_pushgrad(val[:1], grid, lattice, bound, order, ex),
                  _threads(lambda: masked_truth("pushgrad", p["val"][:1], p["grid"], bound, order, ex, shape=lattice)), fv, "pushgrad: val of batch 1")
            check(ops.grid_pushgrad(val, grid[:1], lattice, bound, order, ex),
                  _threads(lambda: masked_truth("pushgrad", p["val"], p["grid"][:1], bound, order, ex, shape=lattice)), fv, "pushgrad: grid of batch 1")
            # strided volumes: the gather is deterministic, so the very bits of the contiguous call
            if dim > 1:
                view = inp.transpose(-1, -2).contiguous().transpose(-1, -2)
            else:
                view = torch.stack([inp, inp + 1], -1)[..., 0]
            assert not view.is_contiguous() and torch.equal(view, inp)
            assert torch.equal(ops.grid_hess(view, grid, bound, order, ex), ref_h), what + ("transposed / strided volume",)
            wide = torch.randn([S.B, 2 * S.C, *lattice], generator=gen).to(DEV, dtype)
            odd = wide[:, 1::2]
            assert odd.stride(1) == 2 * inp.stride(1)
            assert torch.equal(ops.grid_hess(odd, grid, bound, order, ex), ops.grid_hess(odd.contiguous(), grid, bound, order, ex)), what + ("channel stride",)
            # values stored component first (float atomics: held to the bar, not bitwise)
            comp_first = val.movedim(-1, 2).contiguous().movedim(2, -1)
            assert dim == 1 or not comp_first.is_contiguous()
            check(ops.grid_pushgrad(comp_first, grid, lattice, bound, order, ex), want_p, fv, "pushgrad: component-first values")
            # out= with FLAG_ACCUMULATE: the previous contents plus the result
            prev = torch.randn([S.B, S.C, *lattice], generator=gen).double()
            out = prev.to(DEV, dtype)
            held = out.cpu().double().numpy()
            b3, o3 = ops._codes(grid, bound, order)
            got = _hip.scatter("pushgrad", val, grid, list(lattice), b3, o3, ex, flags=_hip.FLAG_ACCUMULATE, out=out)
            assert got.data_ptr() == out.data_ptr()
            check(out, held + want_p, fv, "pushgrad: accumulate")


# ---------------------------------------------------------------------------------------------------------------------
# 4. 16-bit storage: the host upcasts (interpol/_hip.py: gather, scatter), float32 kernels, one narrowing
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_sixteen_bit_inputs(dtype):
    tol = TOL[dtype]
    for dim in (1, 2, 3):
        lattice, samples = S.SHAPES[dim][0]
        p = problem(lattice, samples)
        grid = p["grid"].to(DEV, torch.float32)
        inp, val = p["inp"].to(DEV, dtype), p["val"].to(DEV, dtype)
        inp_up, val_up = inp.float(), val.float()                        # (the oracle sees the stored values)
        for i, order in enumerate((1, 3, 4, 6, 7)):
            bound, ex = (2 * i + dim) % 7, (i + dim) % 3
            what = (str(dtype), dim, order, bound, ex)
            got = ops.grid_hess(inp, grid, [bound], [order], ex)
            assert got.dtype == dtype, what
            want = _threads(lambda: masked_truth("hess", inp_up, p["grid"], [bound], [order], ex))
            r = ratio(got, want, tol, amax(inp_up))
            assert r <= 1.0, what + ("hess", r)
            assert torch.equal(got, ops.grid_hess(inp_up, grid, [bound], [order], ex).to(dtype)), what + ("hess: one narrowing of the float32 result",)
            got = ops.grid_pushgrad(val, grid, lattice, [bound], [order], ex)
            assert got.dtype == dtype, what
            want = _threads(lambda: masked_truth("pushgrad", val_up, p["grid"], [bound], [order], ex, shape=lattice))
            r = ratio(got, want, tol, amax(val_up))
            assert r <= 1.0, what + ("pushgrad", r)


# ---------------------------------------------------------------------------------------------------------------------
# 5. ops.grid_grad_backward itself
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_grid_grad_backward_on_the_device(dim, dtype, monkeypatch):
    """grad_inp = pushgrad(grad), grad_grid = sum_c sum_d hess[..., d, :] grad[..., d] (pushpull.py:303-325).  The floor of the
    grid gradient's bar is the larger of max|inp| and max|grad|."""
    tol = TOL[dtype]
    calls = hip_calls(monkeypatch)
    worst = 0.0
    for case, (lattice, samples) in enumerate(S.SHAPES[dim]):
        p = problem(lattice, samples)
        d = on_device(p, dtype)
        fg, fb = amax(p["grad"]), amax(p["inp"], p["grad"])
        for order in (1, 2, 3, 4, 6):
            for bound in (3, 6, 0, 4):                                   # dct2, dft, zero, dst1
                base = _threads(lambda: np.asarray(oracle.grid_hess(p["inp"], p["grid"], [bound], [order], 1)))
                for ex in (1, 0, 2):
                    what = (lattice, str(dtype), order, bound, ex)
                    if ex == 1:
                        wi, wg = _threads(lambda: oracle.grid_grad_backward(p["grad"].numpy(), p["inp"].numpy(), p["grid"].numpy(), [bound], [order], 1))
                    else:
                        wi, wg = _threads(lambda: masked_truth("grad_backward", p["inp"], p["grid"], [bound], [order], ex, grad=p["grad"], base=base))
                    before = dict(calls)
                    gi, gg = ops.grid_grad_backward(d["grad"], d["inp"], d["grid"], [bound], [order], ex, need_inp=True, need_grid=True)
                    assert (calls.get("pushgrad", 0) - before.get("pushgrad", 0), calls.get("hess", 0) - before.get("hess", 0)) == (1, 1), what
                    assert gi.dtype == dtype and gg.dtype == dtype and list(gi.shape) == [S.B, S.C, *lattice] and list(gg.shape) == [S.B, *samples, dim]
                    ri, rg = ratio(gi, wi, tol, fg), ratio(gg, wg, tol, fb)
                    worst = max(worst, ri, rg)
                    assert ri <= 1.0 and rg <= 1.0, what + ("grad_inp %.3g grad_grid %.3g" % (ri, rg),)
                # one gradient at a time: the other is None and its kernel is not launched
                before = dict(calls)
                gi, none = ops.grid_grad_backward(d["grad"], d["inp"], d["grid"], [bound], [order], ex, need_inp=True, need_grid=False)
                assert none is None and calls.get("hess", 0) == before.get("hess", 0) and calls["pushgrad"] == before["pushgrad"] + 1
                assert ratio(gi, wi, tol, fg) <= 1.0, what
                before = dict(calls)
                none, gg = ops.grid_grad_backward(d["grad"], d["inp"], d["grid"], [bound], [order], ex, need_inp=False, need_grid=True)
                assert none is None and calls["pushgrad"] == before["pushgrad"] and calls["hess"] == before["hess"] + 1
                assert ratio(gg, wg, tol, fb) <= 1.0, what
    print("grid_grad_backward %d-D %s: worst error / allowed = %.4f" % (dim, dtype, worst))


# ---------------------------------------------------------------------------------------------------------------------
# 6. autograd: a double backward whose second pass runs the HIP kernels
# ---------------------------------------------------------------------------------------------------------------------
DB_LATTICE, DB_SAMPLES = (7, 6, 8), (5, 4, 6)


def _first_and_second(op, x, grid, z, kw, create_graph=True):
    """loss = sum y^2; g1 = d loss / d (x, grid) (count: grid alone); -> d <g1, z> / d (x, grid), or g1 itself without a graph"""
    if op == "pull":
        y = interpol.grid_pull(x, grid, **kw)
    elif op == "push":
        y = interpol.grid_push(x, grid, shape=DB_LATTICE, **kw)
    elif op == "count":
        y = interpol.grid_count(grid, shape=DB_LATTICE, **kw)
    else:
        y = interpol.grid_grad(x, grid, **kw)
    wrt = (grid,) if op == "count" else (x, grid)
    g1 = torch.autograd.grad(y.square().sum(), wrt, create_graph=create_graph)
    if not create_graph:
        return g1
    return torch.autograd.grad(sum((g * zz).sum() for g, zz in zip(g1, z)), wrt)


@pytest.mark.parametrize("op", ["pull", "push", "count", "grad"])
def test_double_backward_runs_the_hip_kernels(op, monkeypatch):
    """float64, orders 3 and 5, extrapolate False and True, on the device against the same computation on the CPU with the oracle
    as the kernel table.  pull, push, count: the first backward (create_graph=True) is composed of GridPush / GridPull / GridGrad,
    and the second pass differentiates GridGrad with ops.grid_grad_backward -- hess and pushgrad must be reached.  grid_grad: its
    FIRST backward is grid_grad_backward (asserted on a backward without a graph); under create_graph=True autograd differentiates
    the PyTorch restatement instead (interpol/autograd.py: GridGrad.backward), which is compared too but owes neither kernel."""
    p = problem(DB_LATTICE, DB_SAMPLES)
    gen = torch.Generator().manual_seed(5)
    x0 = p["inp"] if op in ("pull", "grad") else p["val"][..., 0].contiguous()
    g0 = p["grid"]
    z = [torch.randn(t.shape, generator=gen, dtype=torch.float64) for t in ((g0,) if op == "count" else (x0, g0))]
    calls = hip_calls(monkeypatch)
    for order in (3, 5):
        for ex in (False, True):
            kw = dict(interpolation=order, bound="dct2", extrapolate=ex)
            for graph in ([True, False] if op == "grad" else [True]):
                before = dict(calls)
                got = _first_and_second(op, x0.to(DEV).requires_grad_(True), g0.to(DEV).requires_grad_(True), [t.to(DEV) for t in z], kw, graph)
                reached = (calls.get("hess", 0) - before.get("hess", 0), calls.get("pushgrad", 0) - before.get("pushgrad", 0))
                if not (op == "grad" and graph):
                    assert reached[0] >= 1 and reached[1] >= 1, (op, order, ex, reached)
                with ops.use_kernels(OracleKernels):
                    want = _first_and_second(op, x0.clone().requires_grad_(True), g0.clone().requires_grad_(True), z, kw, graph)
                assert len(got) == len(want)
                for a, b in zip(got, want):
                    assert float(b.abs().max()) > 0
                    err = float((a.cpu() - b).abs().max())
                    assert err <= 1e-9 * max(1.0, float(b.abs().max())), (op, order, ex, graph, err)


@pytest.mark.parametrize("ex", [False, True], ids=["masked", "extrapolated"])
@pytest.mark.parametrize("op", ["pull", "push"])
def test_gradgradcheck_on_the_device(op, ex, monkeypatch):
    """Cubic, (4, 3, 5).  Coordinates: an integer plus a fraction in [0.2, 0.8] that keeps 0.06 away from 0.45 and 0.55 -- so at
    least 0.05 away from every knot and from every mask threshold (-0.05, n - 1 + 0.05, -0.55, n - 1 + 0.55 have the fractions
    0.95, 0.05, 0.45, 0.55) and finite differences cross neither.  Every third sample lies one voxel below the lattice in dim 0,
    every sixth one voxel above it in dim 2; the others are inside."""
    lattice, samples = (4, 3, 5), (2, 3, 2)
    gen = torch.Generator().manual_seed(11)
    whole = torch.stack([torch.randint(0, n - 1, [12], generator=gen) for n in lattice], -1).double()
    whole[0::3, 0] = -1
    whole[1::6, 2] = lattice[2] - 1
    frac = 0.2 + 0.6 * torch.rand([12, 3], generator=gen, dtype=torch.float64)
    frac = torch.where((frac - 0.5).abs() < 0.06, frac + 0.12, frac)
    grid = (whole + frac).reshape(1, *samples, 3).to(DEV).requires_grad_(True)
    assert abs(S.masked_share(grid.detach().cpu(), lattice, 0) - 0.5) < 1e-9
    x = torch.randn([1, 1, *(lattice if op == "pull" else samples)], generator=gen, dtype=torch.float64).to(DEV).requires_grad_(True)
    kw = dict(interpolation=3, bound="dct2", extrapolate=ex)
    calls = hip_calls(monkeypatch)
    if op == "pull":
        fn = lambda a, g: interpol.grid_pull(a, g, **kw)
    else:
        fn = lambda a, g: interpol.grid_push(a, g, shape=lattice, **kw)
    assert torch.autograd.gradgradcheck(fn, (x, grid))
    assert calls.get("hess", 0) > 0 and calls.get("pushgrad", 0) > 0


# ---------------------------------------------------------------------------------------------------------------------
# 7. memory contract: what tests/test_memory_contract.py leaves open (1-D and 2-D, float64, orders 1, 4, 6)
# ---------------------------------------------------------------------------------------------------------------------
# dim 0 is the one that is halved: samples stay below n0 // 2 - 5 there, an order-6 stencil reaches 4 voxels further
HALF = {1: ((67,), (300,)), 2: ((22, 13), (19, 11)), 3: ((17, 10, 13), (11, 14, 9))}


def _half_problem(dim):
    lattice, samples = HALF[dim]
    p = dict(problem(lattice, samples, seed=1))
    gen = torch.Generator().manual_seed(40 + dim)
    top = lattice[0] // 2 - 5
    line = S.dyadic_line(top + 3, samples[0], 0.0) - 2                   # -2 .. top
    g = p["grid"].clone()
    g[..., 0] = line.reshape([1, -1] + [1] * (dim - 1)) + torch.randint(-32, 1, g.shape[:-1], generator=gen).double() / 64
    assert float(g[..., 0].max()) <= top and 0.05 < S.masked_share(g, lattice, 0) < 0.9
    p["grid"] = g.contiguous()
    return p, lattice, samples


@pytest.mark.parametrize("misalign", [0, 1, 3])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_memory_contract(dim, dtype, misalign):
    """Poisoned outputs between guards, guarded inputs off 16-byte alignment, ex = 0 (the masked samples multiply what they gathered
    by zero: a read outside the volume would leave a NaN).  Bounds zero, replicate, dct1, dct2 fold a tap that leaves the lattice
    back next to where it left, so with every sample in the lower half of dim 0 no tap reaches the upper half: it must be exactly
    0 -- the zero-fill is the call's own, not inherited from the buffer (which is poisoned)."""
    p, lattice, samples = _half_problem(dim)
    tol = TOL[dtype]
    fi, fv = amax(p["inp"]), amax(p["val"])
    for i, order in enumerate((1, 4, 6)):
        bound = [(0, 1, 2, 3)[(i + dim + k) % 4] for k in range(dim)]
        o = [order] * dim
        what = (dim, str(dtype), order, bound, misalign)
        want_h = _threads(lambda: masked_truth("hess", p["inp"], p["grid"], bound, o, 0))
        want_p = _threads(lambda: masked_truth("pushgrad", p["val"], p["grid"], bound, o, 0, shape=lattice))
        assert not want_p[:, :, lattice[0] // 2:].any() and want_p[:, :, :lattice[0] // 2].any()
        with memguard.installed(_hip, misalign) as seam:
            inp, val, grid = (memguard.place(p[k].to(dtype), DEV, misalign) for k in ("inp", "val", "grid"))
            hess = _hip.gather("hess", inp, grid, bound, o, 0)
            push = _hip.scatter("pushgrad", val, grid, list(lattice), bound, o, 0)
            torch.cuda.synchronize()
            outs = seam.outputs()
            assert len(outs) == 2 and outs[0].tensor.data_ptr() == hess.data_ptr() and outs[1].tensor.data_ptr() == push.data_ptr(), what
            off = (misalign * hess.element_size()) % 16
            assert hess.data_ptr() % 16 == off and push.data_ptr() % 16 == off and inp.data_ptr() % 16 == off, what
            seam.assert_fully_written(hess, None, what + ("hess",))
            seam.assert_fully_written(push, None, what + ("pushgrad",))
            seam.assert_guards_intact(what)
            for t, k in ((inp, "inp"), (val, "val"), (grid, "grid")):
                memguard.assert_guard_intact(t, what + (k,))
                assert torch.equal(t.cpu(), p[k].to(dtype)), what + (k, "input modified")
            assert not bool(push[:, :, lattice[0] // 2:].any()), what + ("the untouched half of the target is not zero",)
            rh, rp = ratio(hess, want_h, tol, fi), ratio(push, want_p, tol, fv)
            assert rh <= 1.0 and rp <= 1.0, what + ("hess %.3g pushgrad %.3g" % (rh, rp),)
