"""The batch loops on the device: more items than a launch has rows of workgroups.

A launch has at most 65 535 rows of workgroups.  Every kernel that puts the batch item on gridDim.y clamps it there and walks the rest of
the batch in `for (b = blockIdx.y; b < B; b += gridDim.y)`.  Each case below runs B = 65 538 items (tests/batch_loops.py): items
65 535 .. 65 537 are the second trip of rows 0 .. 2, every other row makes one trip.  What must be re-formed per trip -- base pointers
from b * stride and strides of 0, LDS that a workgroup reuses, the slot of an item's partial sums, `continue` against `return`, the
scalars the solver keeps per item -- is then held to float64 truth over the WHOLE batch, nothing sampled and nothing masked beyond
what the operator's own test file leaves out.

Truth and bars are those of the operator's own device test, unchanged (TOL 1e-5 float32 / 1e-11 float64 with that file's scales); no
new tolerance is introduced.  Where the project asserts that bits do not depend on the batch, or the kernel is per-sample without
atomics, the whole call is also `torch.equal` to `chunks` of the same call: slices of at most 32 768 items, whose loops make one trip.
Every fused case counts the calls that reach the binding: a silent fall back to the composed form fails the test.

The conditions these comparisons rest on (distinct items, samples in view, `chunks` itself) are asserted without a device by
tests/test_batch_loops_cpu.py.  Every case prints a `BATCH` line; profiles/batch_loops.txt holds them as measured on an MI355X.

What differs from a plain reading of the sections, and why:
  * lcc (7): the float32 cases run at eps = 1, the float64 cases at the default 1e-5.  csrc/lcc.hip stores I = pull(moving) in the
    field's dtype, rounded once; among 65 538 x 5 windows of two or three points some have next to no contrast, den falls to eps, and
    that rounding alone moves the float64 truth by 40 bars at eps = 1e-5 (tests/test_batch_loops_cpu.py measures it without a
    kernel; the device gave the same 39.9).  tests/test_lcc_gpu.py leaves out its group (offset 10, eps 1e-5) for this reason.
  * regulariser_energy (4): tests/test_regulariser_gpu.py states its bar "rtol = tol, with absolute > 0 so that the energy is well
    away from zero"; membrane + bending alone leave the constants in the null space of L, and 0.4 % of the 1-D items have an energy
    below 0.1 sum v^2.  The energy is held to rtol = tol all the same, alone and with absolute = 2 on top, in both precisions.  This is
    the case that found the one kernel fault of this file: reg_energy formed v (L v) in float32 and stood at 55.7 bars on (4,), 1.49
    and 1.07 on (2, 3); it forms them in double now (test_regulariser_energy_of_membrane_and_bending_alone_in_float32).
  * labels (2): neither binding hands float64 coordinates to the library, so the wide kernel runs on float32 coordinates through
    debug bit 2 of the flags, which is how the library selects it.
  * the tiles' decline (9): the library has no query for the organisation a call took; that 65 536 items are served by the generic
    kernels shows in the time alone (0.52 s against 0.014 s for two calls of 32 768 items), which is printed, not asserted.
  * mi (8): `_hip.mi_covered` did not know the limit of 65 535 items, so a call with one more raised INTERPOL_E_SHAPE out of
    `interpol.mi_gauss_newton` instead of taking the composed form; it knows now, and so do the predicates of the two affine terms.
"""
import time

import numpy as np
import pytest
import torch

import interpol
from interpol import _hip, backend, ops
from interpol.torch_kernels import det_closed
from oracle import oracle
import batch_loops as BL
import memguard
import storage_contract as SC
import test_compose_cpu as compose_cpu
import test_jacobian_cpu as jacobian_cpu
import test_lcc_cpu as lcc_cpu
import test_regulariser_cpu as reg_cpu
import test_regulariser_solve_cpu as st
import test_ssd_cpu as ssd_cpu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = {torch.float32: 1e-5, torch.float64: 1e-11}
B = BL.B_LOOP
BOUNDS = jacobian_cpu.BOUNDS
ids = lambda cases: [c[0] for c in cases]


def dev(t):
    return None if t is None else t.to(DEV)


def count_calls(monkeypatch, *names):
    """count the calls that reach the bindings `names` of the library"""
    calls = {n: 0 for n in names}

    def wrap(name, fn):
        def f(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return f

    for n in names:
        monkeypatch.setattr(_hip, n, wrap(n, getattr(_hip, n)))
    return calls


def timed(fn):
    """(result, seconds) of a device call, the device idle before and after"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def worst(got, want, tol, scale):
    """error / bar of |got - want| <= tol |want| + tol scale, the worst element"""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape and bool(torch.isfinite(got).all())
    return float(((got - want).abs() / (tol * want.abs() + tol * scale).clamp_min(1e-300)).max())


def amax(t):
    return float(t.detach().abs().max())


def same(a, b):
    a, b = ((a,), (b,)) if torch.is_tensor(a) else (a, b)
    return len(a) == len(b) and all((x is None and y is None) or (x.shape == y.shape and torch.equal(x, y)) for x, y in zip(a, b))


def oracle_threads(fn):
    oracle.set_threads(8)
    try:
        return fn()
    finally:
        oracle.set_threads(1)


def report(op, name, ratios, bits, calls, seconds, t0):
    print("BATCH %s %s: B %d; error / bar %s; chunks bit-identical: %s; binding calls %s; device call %.3f s, case %.1f s"
          % (op, name, B, ", ".join("%s %.3g" % kv for kv in ratios.items()), bits, calls, seconds, time.perf_counter() - t0))
    assert all(v <= 1.0 for v in ratios.values()), (op, name, ratios)


# ---------------------------------------------------------------------------------------------------------------------
# 3. compose, jacobian and jacdet: forward against the oracle, backward against the float64 composed route
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", BL.COMPOSE_CASES, ids=ids(BL.COMPOSE_CASES))
def test_compose_forward_and_backward(case, monkeypatch):
    t0 = time.perf_counter()
    name, (lshape, oshape), dt, order, bound, ex, lB = case
    dtype, tol = BL.DT[dt], TOL[BL.DT[dt]]
    monkeypatch.setattr(backend, "fused_compose_orders", (1, 2, 3))
    calls = count_calls(monkeypatch, "compose", "compose_backward_right")
    left, right = BL.compose_fields(lshape, oshape, dtype, lB=lB)
    l, r = left.to(DEV), right.to(DEV)
    kw = dict(interpolation=order, bound=bound, extrapolate=ex)
    assert r.shape[0] == B and l.shape[0] == (lB or B) and ops.compose_covered(l, r, [order])
    # forward: the oracle in the fields' dtype (tests/test_compose_gpu.py: oracle_compose), every item
    dim = len(oshape)
    grid = interpol.add_identity_grid(right)
    lcf = left.movedim(-1, 1).contiguous()
    pulled = torch.as_tensor(oracle_threads(lambda: oracle.grid_pull(lcf.expand(B, *lcf.shape[1:]).contiguous(), grid,
                                                                     [BOUNDS.index(bound)] * dim, order, ex))).movedim(1, -1)
    want = (right + pulled).double()
    got, seconds = timed(lambda: interpol.compose(l, r, **kw))
    assert got.shape == r.shape and got.dtype == dtype and calls["compose"] == 1
    ratios = dict(forward=worst(got, want, tol, amax(pulled.double())))
    bits = same(got, BL.chunks(lambda a, b: interpol.compose(a, b, **kw), [l, r]))
    assert bits and calls["compose"] == 4
    # backward: the float64 composed route on the device (tests/test_compose_gpu.py: _grads)
    w = torch.randn(right.shape, generator=torch.Generator().manual_seed(BL.SEED + 2), dtype=torch.float64).to(dtype).to(DEV)

    def grads(f, a, b, c):
        a, b = a.clone().requires_grad_(), b.clone().requires_grad_()
        return torch.autograd.grad((f(a, b, **kw) * c).sum(), (a, b))

    ref_l, ref_r = grads(compose_cpu.composed, l.double().expand(B, *l.shape[1:]), r.double(), w.double())
    if lB:
        ref_l = ref_l.sum(0, keepdim=True)
    got_l, got_r = grads(interpol.compose, l, r, w)
    assert calls["compose"] == 5 and calls["compose_backward_right"] == 1
    ratios["grad_right"] = worst(got_r, ref_r, tol, amax(ref_r))
    ratios["grad_left"] = worst(got_l, ref_l, tol, amax(ref_l))
    report("compose", name, ratios, bits, dict(calls), seconds, t0)


@pytest.mark.parametrize("case", BL.JACOBIAN_CASES, ids=ids(BL.JACOBIAN_CASES))
def test_jacobian_and_jacdet_forward_and_backward(case, monkeypatch):
    t0 = time.perf_counter()
    name, shape, dt, order, bound = case
    dtype, tol = BL.DT[dt], TOL[BL.DT[dt]]
    dim = len(shape)
    monkeypatch.setattr(backend, "fused_jacobian_orders", (1, 2, 3))
    calls = count_calls(monkeypatch, "jacobian", "jacdet_backward_field")
    u = BL.field(shape, dtype, builder=jacobian_cpu)
    ud = u.to(DEV)
    kw = dict(interpolation=order, bound=bound)
    assert ud.shape[0] == B and ops.jacobian_covered(ud, [order])
    wantJ = oracle_threads(lambda: jacobian_cpu.oracle_jacobian(u, BOUNDS.index(bound), order))
    wantd = det_closed(wantJ).double()
    wantJ = wantJ.double()
    (J, d), seconds = timed(lambda: (interpol.jacobian(ud, **kw), interpol.jacdet(ud, **kw)))
    assert J.dtype == dtype and d.dtype == dtype and J.shape == (B, *shape, dim, dim) and d.shape == (B, *shape) and calls["jacobian"] == 2
    ratios = dict(jacobian=worst(J, wantJ, tol, amax(wantJ)), jacdet=worst(d, wantd, tol, amax(wantd)))
    bits = same(J, BL.chunks(lambda x: interpol.jacobian(x, **kw), [ud])) and same(d, BL.chunks(lambda x: interpol.jacdet(x, **kw), [ud]))
    assert bits and calls["jacobian"] == 8
    # backward (the cofactor kernel and the transposed stencil): the float64 composed route on the device
    gen = torch.Generator().manual_seed(BL.SEED + 3)
    w = torch.randn(ud.shape[:-1], generator=gen, dtype=torch.float64).to(DEV)
    W = torch.randn([*ud.shape, dim], generator=gen, dtype=torch.float64).to(DEV)
    r = ud.double().requires_grad_()
    Jr = interpol.grid_grad(r.movedim(-1, 1), torch.zeros_like(r), displacement=True, extrapolate=True, **kw).movedim(1, -2) \
        + torch.eye(dim, dtype=torch.float64, device=DEV)
    ref_d, = torch.autograd.grad((torch.linalg.det(Jr) * w).sum(), r, retain_graph=True)
    ref_J, = torch.autograd.grad((Jr * W).sum(), r)
    v = ud.clone().requires_grad_()
    got_d, = torch.autograd.grad((interpol.jacdet(v, **kw) * w.to(dtype)).sum(), v)
    got_J, = torch.autograd.grad((interpol.jacobian(v, **kw) * W.to(dtype)).sum(), v)
    assert calls["jacdet_backward_field"] == 1 and calls["jacobian"] == 10
    assert amax(ref_d) > 1e-3 * amax(w) and amax(ref_J) > 1e-3 * amax(W)                      # (not the case where every stencil cancels)
    ratios["grad_jacdet"] = worst(got_d, ref_d, tol, amax(ref_d))
    ratios["grad_jacobian"] = worst(got_J, ref_J, tol, amax(ref_J))
    report("jacobian", name, ratios, bits, dict(calls), seconds, t0)


# ---------------------------------------------------------------------------------------------------------------------
# 4. regulariser: matvec, energy and the backward of both against the dense matrix
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", BL.REG_CASES, ids=ids(BL.REG_CASES))
def test_regulariser_matvec_energy_and_their_backward(case, monkeypatch):
    t0 = time.perf_counter()
    name, shape, dt, bound, seed = case
    dtype, tol = BL.DT[dt], TOL[BL.DT[dt]]
    dim = len(shape)
    symmetric = bound in reg_cpu.SYMMETRIC
    calls = count_calls(monkeypatch, "regulariser", "regulariser_energy")
    v, g = BL.field(shape, dtype, seed=seed), BL.field(shape, dtype, seed=seed + 1)
    ge = torch.randn([B], generator=torch.Generator().manual_seed(seed + 2), dtype=torch.float64).to(dtype)
    S = reg_cpu.spatial_matrix(shape, bound, **BL.REG_WEIGHTS)
    kw = dict(bound=bound, **BL.REG_WEIGHTS)
    vd = v.to(DEV)
    assert vd.shape[0] == B and ops.regulariser_covered(vd)
    wantL, wantE = reg_cpu.apply_dense(S, v), reg_cpu.energy_dense(S, v)
    assert amax(wantL) > 0.1 * amax(v)
    (Lv, E), seconds = timed(lambda: (interpol.regulariser(vd, **kw), interpol.regulariser_energy(vd, **kw)))
    assert Lv.dtype == dtype and E.dtype == dtype and E.shape == (B,) and calls == dict(regulariser=1, regulariser_energy=1)
    # the energy at rtol = tol of |want|: membrane + bending alone, and with absolute = 2 on top (the weights under which
    # tests/test_regulariser_gpu.py states that bar: every energy is then well away from zero)
    kwa = dict(kw, absolute=BL.REG_ABSOLUTE)
    wantEa = reg_cpu.energy_dense(reg_cpu.spatial_matrix(shape, bound, absolute=BL.REG_ABSOLUTE, **BL.REG_WEIGHTS), v)
    assert bool((wantEa > 0.1 * v.double().square().reshape(B, -1).sum(1)).all())
    Ea = interpol.regulariser_energy(vd, **kwa)
    ratios = dict(matvec=worst(Lv, wantL, tol, amax(wantL)), energy=worst(E, wantE, tol, 0.0), energy_with_absolute=worst(Ea, wantEa, tol, 0.0))
    bits = same(Lv, BL.chunks(lambda x: interpol.regulariser(x, **kw), [vd])) \
        and same(E, BL.chunks(lambda x: interpol.regulariser_energy(x, **kw), [vd])) \
        and same(Ea, BL.chunks(lambda x: interpol.regulariser_energy(x, **kwa), [vd]))
    assert bits and calls == dict(regulariser=4, regulariser_energy=8)
    # backward: L^T g, and ge (L + L^T) v / 2; the fused kernel where L is symmetric, the transposed composed form where it is not
    x = vd.clone().requires_grad_()
    before = dict(calls)
    got, = torch.autograd.grad(interpol.regulariser(x, **kw), x, g.to(DEV))
    assert calls["regulariser"] - before["regulariser"] == (2 if symmetric else 1)
    want = reg_cpu.apply_dense(S, g, transpose=True)
    ratios["grad_matvec"] = worst(got, want, tol, amax(want))
    before = dict(calls)
    got, = torch.autograd.grad(interpol.regulariser_energy(x, **kw), x, ge.to(DEV))
    assert (calls["regulariser_energy"] - before["regulariser_energy"], calls["regulariser"] - before["regulariser"]) == (1, 1 if symmetric else 0)
    want = 0.5 * (wantL + reg_cpu.apply_dense(S, v, transpose=True)) * ge.double().reshape([B] + [1] * (dim + 1))
    ratios["grad_energy"] = worst(got, want, tol, amax(want))
    report("regulariser", name, ratios, bits, dict(calls), seconds, t0)


F32_REG_CASES = [c for c in BL.REG_CASES if c[2] == "f32"]


@pytest.mark.parametrize("case", F32_REG_CASES, ids=ids(F32_REG_CASES))
def test_regulariser_energy_of_membrane_and_bending_alone_in_float32(case, monkeypatch):
    """The float32 energy of membrane + bending alone against the dense matrix at rtol = 1e-5 of |want|, every item: the case that
    showed that reg_energy (csrc/regulariser.hip) must not form v_d (L v)_d in float32.  Without `absolute` the constants are in the
    null space of L under these bounds; the energy of a nearly constant item is next to zero while the products that sum to it are
    not, and their float32 rounding -- some 1e-7 of sum |coefficient| |v|^2, about 89 sum v^2 in 2-D at these weights -- stood at 55.7
    bars on (4,) dct2, 1.49 on (2, 3) dct2 and 1.07 on (2, 3) replicate (worst item of 65 538; 0.048 on (2, 3, 2)), on the whole
    batch and on its slices alike: no fault of the loop, but of every smooth field, whose taps cancel the same way.  The kernel now
    forms the coefficients, the products and the sum in double for a float32 field too; measured on an MI355X every case is at
    0.006 of the bar, the one rounding of the result."""
    name, shape, dt, bound, seed = case
    calls = count_calls(monkeypatch, "regulariser_energy")
    v = BL.field(shape, torch.float32, seed=seed)
    vd = v.to(DEV)
    kw = dict(bound=bound, **BL.REG_WEIGHTS)
    wantE = reg_cpu.energy_dense(reg_cpu.spatial_matrix(shape, bound, **BL.REG_WEIGHTS), v)
    E = interpol.regulariser_energy(vd, **kw)
    assert same(E, BL.chunks(lambda x: interpol.regulariser_energy(x, **kw), [vd])) and calls["regulariser_energy"] == 4
    ratio = worst(E, wantE, 1e-5, 0.0)
    print("BATCH regulariser_energy_f32_alone %s: B %d; error / bar energy %.3g; chunks bit-identical: True; binding calls %s"
          % (name, B, ratio, dict(calls)))
    assert ratio <= 1.0, (name, ratio)


# ---------------------------------------------------------------------------------------------------------------------
# 5. regulariser_solve: fixed counts against the restated algorithm, and items that stop on their own count
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", BL.SOLVE_CASES, ids=ids(BL.SOLVE_CASES))
def test_regulariser_solve_fixed_count_and_early_stops(case, monkeypatch):
    t0 = time.perf_counter()
    name, shape, dt, bound, kind = case
    dtype, tol = BL.DT[dt], TOL[BL.DT[dt]]
    calls = count_calls(monkeypatch, "regulariser_solve")
    sy = BL.solve_system(shape, bound, BL.SOLVE_WEIGHTS, 1., kind, dtype)
    g, h = dev(sy["g"]), dev(sy["h"])
    assert g.shape[0] == B and (h is None or h.shape[0] == B) and ops.regulariser_solve_covered(g, h)
    want = BL.restated_batch(sy, 4).reshape(sy["g"].shape)
    kw = dict(max_iter=4, tolerance=0., return_info=True, **sy["kw"])
    (x, info), seconds = timed(lambda: interpol.regulariser_solve(g, h, **kw))
    assert x.dtype == dtype and x.shape == g.shape and info.iterations.shape == (B,) and bool((info.iterations <= 4).all())
    assert calls["regulariser_solve"] == 1
    ratios = dict(x=st.close(x, want, tol))

    def flat(fn):
        def f(a, b):
            y, i = fn(a, b)
            return y, i.iterations, i.residual
        return f

    solve = flat(lambda a, b: interpol.regulariser_solve(a, b, **kw))
    bits = same((x, info.iterations, info.residual), BL.chunks(solve, [g, h]))
    assert bits and calls["regulariser_solve"] == 4
    # a tolerance that stops some items early and not others: every item of the second trip stops on its own count
    kw = dict(kw, max_iter=BL.EARLY_MAX_ITER, tolerance=BL.EARLY_TOLERANCE)
    solve = flat(lambda a, b: interpol.regulariser_solve(a, b, **kw))
    whole = solve(g, h)
    its = whole[1].cpu()
    stopped = float((its < BL.EARLY_MAX_ITER).double().mean())
    assert 0.1 < stopped < 0.9, stopped                                  # (tests/test_batch_loops_cpu.py: from the truth alone)
    early = same(whole, BL.chunks(solve, [g, h]))
    assert early and calls["regulariser_solve"] == 8
    print("BATCH regulariser_solve %s: tolerance %g, max_iter %d: %.3f of the items stop early; iterations of the pinned items %s"
          % (name, BL.EARLY_TOLERANCE, BL.EARLY_MAX_ITER, stopped, its[list(BL.PINNED)].tolist()))
    report("regulariser_solve", name, ratios, bits and early, dict(calls), seconds, t0)


# ---------------------------------------------------------------------------------------------------------------------
# 6. ssd_gauss_newton
# ---------------------------------------------------------------------------------------------------------------------
def ssd_truth(case):
    def make():
        args, kw = BL.ssd_case(case)
        return args, kw, ssd_cpu.reference(*args, **kw), ssd_cpu.scales(*[args[i] for i in (0, 1, 3)])
    return BL.cached(("ssd", case[0]), make)


@pytest.mark.parametrize("case", BL.SSD_CASES, ids=ids(BL.SSD_CASES))
def test_ssd_gauss_newton(case, monkeypatch):
    t0 = time.perf_counter()
    name, dim, dt, order, bound, ex, sigma, hessian, own, seed = case
    dtype, tol = BL.DT[dt], TOL[BL.DT[dt]]
    monkeypatch.setattr(backend, "fused_ssd_orders", (1, 2, 3))
    monkeypatch.setattr(backend, "fused_ssd_orders_without_hessian", (1, 2, 3))
    calls = count_calls(monkeypatch, "ssd")
    args, kw, want, (sg, sh) = ssd_truth(case)
    moving, fixed, disp, weight = [dev(t) for t in args]
    assert moving.shape[:2] == (B, 2) and fixed.shape[0] == (B if own else 2) and disp.shape[0] == B and weight.shape[0] == B
    if not ex:
        assert ssd_cpu.in_view(args[2], BL.SSD_LATTICES[dim][0]) >= 0.20
    fn = lambda m, f, u, w: interpol.ssd_gauss_newton(m, f, u, w, **kw)
    got, seconds = timed(lambda: fn(moving, fixed, disp, weight))
    assert calls["ssd"] == 1 and got[0].shape == (B,) and got[1].shape == disp.shape and all(t.dtype == dtype for t in got if t is not None)
    ratios = dict(loss=worst(got[0], want[0], tol, 0.0), gradient=worst(got[1], want[1], tol, sg))
    if hessian is None:
        assert got[2] is None
    else:
        assert got[2].shape == want[2].shape
        ratios["hessian"] = worst(got[2], want[2], tol, sh)
    bits = same(got, BL.chunks(fn, [moving, fixed, disp, weight]))
    assert bits and calls["ssd"] == 4
    report("ssd", name, ratios, bits, dict(calls), seconds, t0)


# ---------------------------------------------------------------------------------------------------------------------
# 7. lcc_gauss_newton
# ---------------------------------------------------------------------------------------------------------------------
def lcc_truth(case):
    def make():
        args, kw = BL.lcc_case(case)
        return args, kw, lcc_cpu.truth(*args, **kw)
    return BL.cached(("lcc", case[0]), make)


def lcc_worst(got, want, tol, with_scale=True):
    """tests/test_lcc_cpu.py: item_ratio -- the scale is max |want| of the ITEM -- without its loop over the items"""
    got, want = got.detach().cpu().double(), want.double()
    assert got.shape == want.shape and bool(torch.isfinite(got).all())
    scale = want.abs().flatten(1).max(1).values.reshape([-1] + [1] * (want.dim() - 1)) if with_scale else 0.0
    return float(((got - want).abs() / (tol * scale + tol * want.abs()).clamp_min(1e-300)).max())


@pytest.mark.parametrize("case", BL.LCC_CASES, ids=ids(BL.LCC_CASES))
def test_lcc_gauss_newton(case, monkeypatch):
    t0 = time.perf_counter()
    name, dim, dt, order, bound, ex, sigma, window, hessian, seed, eps = case
    dtype, tol = BL.DT[dt], TOL[BL.DT[dt]]
    monkeypatch.setattr(backend, "fused_lcc_orders", (1, 2, 3))
    calls = count_calls(monkeypatch, "lcc")
    args, kw, want = lcc_truth(case)
    moving, fixed, disp, weight = [dev(t) for t in args]
    assert moving.shape[:2] == (B, 2) and fixed.shape[0] == 2 and disp.shape[0] == B and weight.shape[0] == B
    if not ex:
        assert ssd_cpu.in_view(args[2], BL.LCC_LATTICES[dim][0]) >= 0.20
    assert want[3] > 1e-3                                               # (mean cc: not zeros against zeros)
    fn = lambda m, f, u, w: interpol.lcc_gauss_newton(m, f, u, w, **kw)
    got, seconds = timed(lambda: fn(moving, fixed, disp, weight))
    assert calls["lcc"] == 1 and got[0].shape == (B,) and got[1].shape == disp.shape and all(t.dtype == dtype for t in got if t is not None)
    # one item against the loop of item_ratio: the vectorised form above is that bar
    assert abs(lcc_worst(got[1][:3], want[1][:3], tol) - lcc_cpu.item_ratio(got[1][:3], want[1][:3], tol)) <= 1e-9
    ratios = dict(loss=lcc_worst(got[0], want[0], tol, False), gradient=lcc_worst(got[1], want[1], tol))
    if hessian is None:
        assert got[2] is None
    else:
        assert got[2].shape == want[2].shape
        ratios["hessian"] = lcc_worst(got[2], want[2], tol)
    bits = same(got, BL.chunks(fn, [moving, fixed, disp, weight]))
    assert bits and calls["lcc"] == 4
    report("lcc", name, ratios, bits, dict(calls), seconds, t0)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the generic kernels: pull, grad, push, count, their backward passes, and hess / pushgrad behind the backward of grid_grad
# ---------------------------------------------------------------------------------------------------------------------
def hip_calls(monkeypatch):
    """count the calls that reach the two entry points of the host layer, by operator (tests/test_second_order_gpu.py)"""
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


def generic_truth(case):
    """the C oracle in float64 (masked Hessians: the identity of tests/test_second_order_cpu.py), once per case"""
    import test_second_order_cpu as S
    name, dim, dt, order, bound, ex = case

    def make():
        p = BL.generic_problem(dim)
        b, o = [BOUNDS.index(bound)], [order]
        n = {k: v.numpy() for k, v in p.items() if torch.is_tensor(v)}
        t = dict(pull=oracle.grid_pull(n["inp"], n["grid"], b, o, ex), grad=oracle.grid_grad(n["inp"], n["grid"], b, o, ex),
                 push=oracle.grid_push(n["val"], n["grid"], p["lattice"], b, o, ex), count=oracle.grid_count(n["grid"], p["lattice"], b, o, ex))
        t["pull_bwd_inp"], t["pull_bwd_grid"] = oracle.grid_pull_backward(n["val"], n["inp"], n["grid"], b, o, ex)
        t["push_bwd_val"], t["push_bwd_grid"] = oracle.grid_push_backward(n["gout"], n["val"], n["grid"], b, o, ex)
        t["grad_bwd_inp"], t["grad_bwd_grid"] = S.masked_truth("grad_backward", p["inp"], p["grid"], b, o, ex, grad=p["grad"])
        return p, {k: torch.as_tensor(np.asarray(v)) for k, v in t.items()}
    return BL.cached(("generic", name), lambda: oracle_threads(make))


@pytest.mark.parametrize("case", BL.GENERIC_CASES, ids=ids(BL.GENERIC_CASES))
def test_generic_kernels(case, monkeypatch):
    t0 = time.perf_counter()
    name, dim, dt, order, bound, ex = case
    dtype, tol = BL.DT[dt], TOL[BL.DT[dt]]
    calls = hip_calls(monkeypatch)
    p, want = generic_truth(case)
    d = {k: (v.to(DEV, dtype) if torch.is_tensor(v) else v) for k, v in p.items()}
    kw = dict(interpolation=order, bound=bound, extrapolate=ex)
    lattice = p["lattice"]
    assert d["inp"].shape[:2] == (B, 2) and d["grid"].shape[0] == B and int(np.prod(p["samples"])) < 4096
    ratios = {}

    def hold(key, got):
        assert got.dtype == dtype
        ratios[key] = worst(got, want[key], tol, amax(want[key]))       # rtol 1e-5, atol 1e-5 max|ref| (golden_util.fp32_tol)

    def once(op, fn):
        """the forward reaches the host layer's entry of `op` exactly once"""
        before = calls.get(op, 0)
        out = fn()
        assert calls.get(op, 0) - before == 1, (op, calls)
        return out

    x, g = d["inp"].clone().requires_grad_(), d["grid"].clone().requires_grad_()
    y, seconds = timed(lambda: once("pull", lambda: interpol.grid_pull(x, g, **kw)))
    hold("pull", y)
    gx, gg = torch.autograd.grad(y, (x, g), d["val"])
    hold("pull_bwd_inp", gx), hold("pull_bwd_grid", gg)
    G_ = once("grad", lambda: interpol.grid_grad(x, g, **kw))
    hold("grad", G_)
    before = dict(calls)
    gx, gg = torch.autograd.grad(G_, (x, g), d["grad"])                 # the backward of grid_grad: pushgrad and hess
    assert (calls.get("pushgrad", 0) - before.get("pushgrad", 0), calls.get("hess", 0) - before.get("hess", 0)) == (1, 1)
    hold("grad_bwd_inp", gx), hold("grad_bwd_grid", gg)
    v = d["val"].clone().requires_grad_()
    z = once("push", lambda: interpol.grid_push(v, g, shape=lattice, **kw))
    hold("push", z)
    gv, gg = torch.autograd.grad(z, (v, g), d["gout"])
    hold("push_bwd_val", gv), hold("push_bwd_grid", gg)
    hold("count", once("count", lambda: interpol.grid_count(d["grid"], shape=lattice, **kw)))
    # per sample, no atomics: pull, grad and hess to the bits of the chunks
    inp, grid = d["inp"], d["grid"]
    hess = lambda a, b: ops.grid_hess(a, b, [BOUNDS.index(bound)], [order], ex)
    bits = same(y.detach(), BL.chunks(lambda a, b: interpol.grid_pull(a, b, **kw), [inp, grid])) \
        and same(G_.detach(), BL.chunks(lambda a, b: interpol.grid_grad(a, b, **kw), [inp, grid])) \
        and same(hess(inp, grid), BL.chunks(hess, [inp, grid]))
    assert bits
    report("generic", name, ratios, bits, dict(calls), seconds, t0)


def test_generic_pull_in_bf16(monkeypatch):
    """one bf16 pull against the bar of the storage contract (tests/storage_contract.py): truth from the STORED inputs"""
    t0 = time.perf_counter()
    calls = hip_calls(monkeypatch)
    p = BL.generic_problem(3)
    inp = p["inp"].to(torch.bfloat16)
    grid = p["grid"].float()
    want = np.asarray(oracle_threads(lambda: oracle.grid_pull(inp.double().numpy(), p["grid"].numpy(), [3], [1], 1)))
    fn = lambda a, b: interpol.grid_pull(a, b, interpolation=1, bound="dct2", extrapolate=True)
    got, seconds = timed(lambda: fn(inp.to(DEV), grid.to(DEV)))
    assert got.dtype == torch.bfloat16 and got.shape[0] == B and calls["pull"] == 1
    bits = same(got, BL.chunks(fn, [inp.to(DEV), grid.to(DEV)]))
    assert bits
    report("generic", "3d-bf16-o1-dct2-ex1-pull", dict(pull=SC.ratio(got.double().cpu().numpy(), want, "bf16")), bits, dict(calls), seconds, t0)


# ---------------------------------------------------------------------------------------------------------------------
# 2. label maps
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", BL.LABEL_CASES, ids=ids(BL.LABEL_CASES))
def test_label_maps(case, monkeypatch):
    """`_hip.pull_labels` on the whole batch against the loop over labels through the float pull, taken in chunks
    (tests/test_hip_parity.py: test_label_map_fused_matches_loop): every label of every item, `torch.equal`"""
    t0 = time.perf_counter()
    name, dim, order, ishape, oshape, gdt, labels = case
    calls = count_calls(monkeypatch, "pull_labels")
    lab, grid = BL.label_problem(case)
    lab, grid = lab.to(DEV), grid.to(DEV)
    assert lab.shape[0] == B and grid.shape[0] == B and _hip.labels_covered(dim, [order] * dim)
    flags = 0
    if gdt == "f64":
        # Neither binding hands float64 coordinates to the library (interpol_pull_labels: INTERPOL_E_DTYPE), so the wide kernel,
        # instantiated for them, is reachable with float32 coordinates alone: debug bit 2 of the flags (csrc/labels.hip: launch_g)
        # sends the 3-D cubic to it instead of the hash kernel.  Same map, same coordinates rounded to float32.
        with pytest.raises(TypeError, match="float32 coordinates"):
            _hip.pull_labels(lab[:1], grid[:1], [3] * dim, [order] * dim, 1)
        grid, flags = grid.float(), 2 << 8
    worst_mism, n = 0.0, 0
    for bound, ex in ((3, 1), (6, 0), (0, 1)):
        opt = ([bound] * dim, [order] * dim, ex)
        fused, seconds = timed(lambda: _hip.pull_labels(lab, grid, *opt, flags=flags))
        n += 1
        assert fused.shape == (B, 2, *oshape)

        def loop(l, g):
            out = torch.zeros([l.shape[0], 2, *oshape], dtype=torch.long, device=DEV)
            pmax = torch.zeros(out.shape, dtype=g.dtype, device=DEV)
            for k in range(labels):
                soft = _hip.gather("pull", (l == k).to(g.dtype), g, *opt, flags=_hip.FLAG_NO_FASTPATH)
                out[soft > pmax] = k
                pmax = torch.max(pmax, soft)
            return out

        want = BL.chunks(loop, [lab, grid])
        mism = float((fused.long() != want).double().mean())
        worst_mism = max(worst_mism, mism)
        assert same(fused, BL.chunks(lambda l, g: _hip.pull_labels(l, g, *opt, flags=flags), [lab, grid])), (name, bound, ex)
        n += 3
        assert torch.equal(fused.long(), want), (name, bound, ex, mism, int((fused.long() != want).sum()))
        assert len(fused.unique()) == labels
    assert calls["pull_labels"] == n + (gdt == "f64")
    report("labels", name, dict(mismatch=worst_mism), True, dict(calls), seconds, t0)


# ---------------------------------------------------------------------------------------------------------------------
# 8. mi_gauss_newton: every item on its own row, the most the library takes; one more is refused
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order,dt", [(1, "f32"), (3, "f32"), (3, "f64")], ids=["o1-f32", "o3-f32", "o3-f64"])
def test_mi_gauss_newton_at_the_edge_of_the_launch(order, dt, monkeypatch):
    import test_mi_cpu as mi_cpu
    import test_mi_gpu as mi_gpu
    t0 = time.perf_counter()
    dtype, tol = BL.DT[dt], TOL[BL.DT[dt]]
    monkeypatch.setattr(backend, "fused_mi_orders", (1, 2, 3))
    calls = count_calls(monkeypatch, "mi")
    moving, fixed, disp, weight = BL.mi_problem(order, dtype)
    assert moving.shape[0] == BL.B_EDGE == 65535 and mi_gpu.no_sample_near_a_bin_edge(fixed, BL.MI_BINS)
    kw = dict(interpolation=order, bound="dct2", extrapolate=True, hessian="full", bins=BL.MI_BINS, moving_range=None,
              fixed_range=(0, BL.MI_BINS - 1), return_histogram=True)
    fn = lambda m, f, u, w: interpol.mi_gauss_newton(m, f, u, w, **kw)
    args = [dev(t) for t in (moving, fixed, disp, weight)]
    got, seconds = timed(lambda: fn(*args))
    assert calls["mi"] == 1 and got[0].shape == (BL.B_EDGE,) and got[3].shape == (BL.B_EDGE, BL.MI_BINS, BL.MI_BINS)
    bits = same(got, BL.chunks(fn, args))
    assert bits and calls["mi"] == 3
    at = [0, 1, BL.B_EDGE - 2, BL.B_EDGE - 1]
    tkw = {k: v for k, v in kw.items() if k != "return_histogram"}
    want, allow, keep = mi_cpu.truth_and_allowance(moving[at], fixed[at], disp[at], weight[at], tol, **tkw)
    assert int((want[0] < -1e-3).sum()) >= 3 and float(want[1].abs().max()) > 0.1          # (not zeros against zeros)
    ratios = mi_gpu.check([t[at] for t in got], want, allow, keep, "batch loops order %d %s" % (order, dt))
    print("BATCH mi o%d-%s: B %d; error / allowance %s (items %s); chunks bit-identical: %s; binding calls %s; device call %.3f s, case %.1f s"
          % (order, dt, BL.B_EDGE, ", ".join("%s %.3g" % kv for kv in ratios.items()), at, bits, dict(calls), seconds, time.perf_counter() - t0))


def test_mi_gauss_newton_refuses_one_item_more_and_the_call_takes_the_composed_form(monkeypatch):
    import ctypes
    import test_mi_gpu as mi_gpu
    from interpol import torch_kernels
    E_SHAPE = -5                                                        # INTERPOL_E_SHAPE
    monkeypatch.setattr(backend, "fused_mi_orders", (1, 2, 3))
    n, bins, dim = BL.B_EDGE + 1, BL.MI_BINS, 3
    moving, fixed, disp, weight = [dev(t) for t in BL.mi_problem(1, torch.float32, B=n)]
    shape = list(BL.MI_LATTICE[1])
    N = int(np.prod(shape))
    # through the real binding, with real operands of 65 536 items: refused before anything is launched
    L = _hip.lib()
    ranges = torch_kernels.mi_ranges(moving, fixed, weight, None, (0, bins - 1), n)
    sentinel = 4321.0
    loss, grad = torch.full([n], sentinel, device=DEV), torch.full([n, *shape, dim], sentinel, device=DEV)
    hess, hist = torch.full([n, *shape, 6], sentinel, device=DEV), torch.full([n, bins, bins], sentinel, device=DEV)
    for items, rc in ((n, E_SHAPE), (n - 1, 0)):
        p = _hip._ssd_problem(moving[:items], fixed[:items], disp[:items], [3] * dim, [1] * dim, 0, items)
        need = L.interpol_mi_workspace(ctypes.byref(p), bins)
        assert need == (E_SHAPE if rc else items * (2 * bins * bins * 8 + 8))
        ws = torch.zeros(max(need, 8), dtype=torch.uint8, device=DEV)
        assert mi_gpu.raw_call(L, p, moving, fixed, disp, weight, ranges, loss, grad, hess, hist, 2, bins, N, dim * N, 6 * N, ws) == rc
        torch.cuda.synchronize()
        assert bool((loss[:items] == sentinel).all()) == bool(rc) and bool((loss[items:] == sentinel).all())
    # the host layer knows: the call does not reach the binding and is served by the composed form
    calls = count_calls(monkeypatch, "mi")
    kw = dict(interpolation=1, bound="dct2", extrapolate=False, bins=bins, fixed_range=(0, bins - 1))
    fewer = [t[:-1] for t in (moving, fixed, disp, weight)]
    assert not ops.mi_covered(moving, fixed, disp, weight, [1], bins) and ops.mi_covered(*fewer, [1], bins)
    got = interpol.mi_gauss_newton(moving, fixed, disp, weight, **kw)
    assert calls["mi"] == 0 and got[0].shape == (n,) and got[1].shape == (n, *shape, dim)
    # (the two affine terms have the item on a row as well -- csrc/data_term.hpp: problem_params; a batch of that size needs 39 GB
    # of workspace there and is not run, but their host layer must know the limit just the same)
    mat = torch.eye(3, 4, device=DEV).expand(n, 3, 4)
    fewer_mat = [fewer[0], fewer[1], mat[:-1], fewer[3]]
    assert not ops.ssd_affine_covered(moving, fixed, mat, weight, [1]) and ops.ssd_affine_covered(*fewer_mat, [1])
    assert not ops.mi_affine_covered(moving, fixed, mat, weight, [1], bins) and ops.mi_affine_covered(*fewer_mat, [1], bins)
    at = [0, 1, n - 2, n - 1]
    want = interpol.mi_gauss_newton(*[t[at].cpu().double() for t in (moving, fixed, disp, weight)], **kw)
    for g, w in zip(got, want):                                         # (the composed form in float32: tests/test_mi_gpu.py, uncovered classes)
        assert float((g[at].double().cpu() - w).abs().max()) <= 1e-4 * float(w.abs().max())
    interpol.mi_gauss_newton(*fewer, **kw)
    assert calls["mi"] == 1                                             # (the control: one item fewer reaches the binding)
    print("BATCH mi one-item-more: B %d refused with INTERPOL_E_SHAPE by interpol_mi and interpol_mi_workspace; the call took the composed form"
          % n)


# ---------------------------------------------------------------------------------------------------------------------
# 10. memory contract: poisoned outputs between guard bands (tests/memguard.py), one case each of sections 1, 3, 6 and 7
# ---------------------------------------------------------------------------------------------------------------------
def _guarded_call(call, args, n_out, n_ws, what):
    """`call(*args)` on ordinary buffers, then on inputs placed between guards with outputs from the poisoned seam: every element
    written, no band touched, the very bits of the ordinary call; -> the guarded outputs"""
    ref = call(*[dev(t) for t in args])
    ref = (ref,) if torch.is_tensor(ref) else tuple(ref)
    assert all(bool(torch.isfinite(r).all()) for r in ref)
    with memguard.installed(_hip, misalign=1) as seam:
        placed = [memguard.place(t, DEV, misalign=1) for t in args]
        out = call(*placed)
        out = (out,) if torch.is_tensor(out) else tuple(out)
        torch.cuda.synchronize()
        assert len(seam.outputs()) == n_out and len(seam.workspaces()) == n_ws, (what, len(seam.outputs()), len(seam.workspaces()))
        assert n_ws == 0 or seam.workspace_was_written(), what
        for t, r in zip(out, ref):
            assert t.shape[0] == B and t.data_ptr() % memguard.ALIGN == t.element_size(), what
            seam.assert_fully_written(t, r, what)
            assert torch.equal(t, r), what
        seam.assert_guards_intact(what)
        for t, a in zip(placed, args):
            memguard.assert_guard_intact(t, what)
            assert torch.equal(t.cpu(), a), what
        return [t.clone() for t in out]


@pytest.mark.parametrize("what", ["generic", "compose", "ssd", "lcc"])
def test_memory_contract(what):
    t0 = time.perf_counter()
    if what == "generic":
        p = BL.generic_problem(3)
        inp, grid = p["inp"].float(), p["grid"].float()
        opt = ([3] * 3, [1] * 3, 1)
        _guarded_call(lambda a, g: _hip.gather("pull", a, g, *opt), [inp, grid], 1, 0, "pull")
        _guarded_call(lambda a, g: _hip.gather("grad", a, g, *opt), [inp, grid], 1, 0, "grad")
        _guarded_call(lambda a, g: _hip.gather("hess", a, g, *opt), [inp, grid], 1, 0, "hess")
    elif what == "compose":
        name, (lshape, oshape), dt, order, bound, ex, lB = BL.COMPOSE_CASES[5]
        left, right = BL.compose_fields(lshape, oshape, BL.DT[dt])
        gout = BL.field(oshape, BL.DT[dt], seed=BL.SEED + 4)
        b, o = [BOUNDS.index(bound)] * 3, [order] * 3
        _guarded_call(lambda l, r: _hip.compose(l, r, b, o, ex), [left, right], 1, 0, name)
        _guarded_call(lambda g, l, r: _hip.compose_backward_right(g, l, r, b, o, ex), [gout, left, right], 1, 0, name + " backward")
    elif what == "ssd":
        case = BL.SSD_CASES[7]
        args, kw, want, _ = ssd_truth(case)
        assert args[1].dim() == 4                                        # (the binding takes fixed as (B | 1, C, *shape))
        args = [args[0], args[1][None], args[2], args[3]]
        opt = ([BOUNDS.index(case[4])] * 3, [case[3]] * 3, int(case[5]), "full")
        loss = _guarded_call(lambda *a: _hip.ssd(*a, *opt), args, 3, 1, case[0])[0]
        # the loss of item 65 537 sits in element 65 537
        last = B - 1
        assert worst(loss[last:], want[0][last:], 1e-5, 0.0) <= 1.0 and worst(loss[:1], want[0][:1], 1e-5, 0.0) <= 1.0
        assert abs(float(want[0][last]) - float(want[0][last - BL.ROWS])) > 1e-3 * abs(float(want[0][last]))
    else:
        case = BL.LCC_CASES[5]
        args, kw, want = lcc_truth(case)
        args = [args[0], args[1][None], args[2], args[3]]
        opt = ([BOUNDS.index(case[4])] * 3, [case[3]] * 3, int(case[5]), "full", [case[7]] * 3, case[10])
        loss = _guarded_call(lambda *a: _hip.lcc(*a, *opt), args, 3, 1, case[0])[0]
        last = B - 1
        assert worst(loss[last:], want[0][last:], 1e-5, 0.0) <= 1.0 and worst(loss[:1], want[0][:1], 1e-5, 0.0) <= 1.0
        assert abs(float(want[0][last]) - float(want[0][last - BL.ROWS])) > 1e-3 * abs(float(want[0][last]))
    print("BATCH memory_contract %s: B %d; every output element written, no guard band touched, the bits of ordinary buffers; case %.1f s"
          % (what, B, time.perf_counter() - t0))


# ---------------------------------------------------------------------------------------------------------------------
# 9. the three-dimensional tiles decline above 65 535 items and hand the call to the generic kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["pull", "push"])
def test_the_tiles_decline_above_65535_items(op):
    """One cubic dct2 float32 call of 65 536 items of 16^3 samples from (into) 8^3 volumes: 4 096 samples per item is what the tiles
    (csrc/ops_sorted.hip: sorted_order, csrc/ops_tiled.hip: tiled_pick) need, so the same call on 32 768 items can take them and on
    65 536 cannot.  Everything is built on the device (3.2 GB of coordinates, 1.1 GB of values).  Against `chunks` at the float32 bar
    (the organisations differ: not bit for bit) and against the oracle on the items 0, 1, 65 534 and 65 535."""
    t0 = time.perf_counter()
    n, lat, smp = 65536, [8, 8, 8], [16, 16, 16]
    gen = torch.Generator(device=DEV).manual_seed(BL.SEED)
    lin = torch.linspace(-0.25, 7.25, 16, device=DEV)
    grid = torch.stack(torch.meshgrid(lin, lin, lin, indexing="ij"), -1)[None] + 0.75 * torch.randn([n, *smp, 3], generator=gen, device=DEV)
    src = torch.randn([n, 1, *(lat if op == "pull" else smp)], generator=gen, device=DEV)
    kw = dict(interpolation=3, bound="dct2", extrapolate=True)
    if op == "pull":
        fn = lambda a, g: interpol.grid_pull(a, g, **kw)
    else:
        fn = lambda a, g: interpol.grid_push(a, g, shape=lat, **kw)
    got, seconds = timed(lambda: fn(src, grid))
    assert got.shape == (n, 1, *(smp if op == "pull" else lat))
    at = [0, 1, n - 2, n - 1]
    s64, g64 = src[at].cpu().double().numpy(), grid[at].cpu().double().numpy()
    want = np.asarray(oracle.grid_pull(s64, g64, [3], [3], 1) if op == "pull" else oracle.grid_push(s64, g64, lat, [3], [3], 1))
    ratios = dict(oracle_on_four_items=worst(got[at], torch.as_tensor(want), 1e-5, float(np.abs(want).max())))
    parts, chunk_seconds = timed(lambda: BL.chunks(fn, [src, grid]))
    del grid
    scale = amax(parts)
    err = (got - parts).abs_()
    del got
    ratios["chunks"] = float((err / (1e-5 * parts.abs_() + 1e-5 * scale)).max())
    print("BATCH tiles_decline %s: B %d; error / bar %s; device call %.3f s (two chunks of 32 768: %.3f s), case %.1f s"
          % (op, n, ", ".join("%s %.3g" % kv for kv in ratios.items()), seconds, chunk_seconds, time.perf_counter() - t0))
    assert all(v <= 1.0 for v in ratios.values()), (op, ratios)
