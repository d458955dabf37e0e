"""The conditions tests/test_batch_loops_gpu.py rests on, asserted from the inputs and the float64 truth alone (no device).

1. Under extrapolate = False with sigma = 0.4 enough samples of every lattice are in view: the comparison is not zeros against zeros.
   Measured with seed 7, float32, after `nudged(disp, 3)`, B = 65 538: SSD lattices 0.885 (1-D), 0.653 (2-D), 0.218 (3-D); the LCC
   lattices of 1-D and 2-D are larger (0.909, 0.750).  The condition is >= 0.20; if the seed changes, re-measure.
2. No two of the items 0, 1, 2, 65 535, 65 536, 65 537 -- rows 0 .. 2 of the launch on their first and on their second trip -- have
   equal truth in any output: they differ by more than 100 times the bar the device test holds that output to.  A kernel that
   mixes up b and b - 65 535, or that computes the second trip from the first trip's operands, cannot pass.
3. `chunks` of the composed CPU form is the composed CPU form of the whole batch, bit for bit; `restated_batch` is `restated`.
   These check the helper, not the library.
"""
import itertools

import pytest
import torch

import interpol
import batch_loops as BL
import test_compose_cpu as compose_cpu
import test_jacobian_cpu as jacobian_cpu
import test_lcc_cpu as lcc_cpu
import test_regulariser_cpu as reg_cpu
import test_regulariser_solve_cpu as st
import test_ssd_cpu as ssd_cpu

F32 = torch.float32
TOL32 = 1e-5
PINNED = list(BL.PINNED)


def test_the_batch_is_three_past_the_rows_of_a_launch():
    assert BL.ROWS == 65535 and BL.B_LOOP == 65538 and BL.B_EDGE == 65535
    assert BL.PINNED == (0, 1, 2, 65535, 65536, 65537)
    assert [b - BL.ROWS for b in BL.SECOND_TRIP] == [0, 1, 2]
    assert BL.B_LOOP > 2 * 32768                                        # three chunks, each below the rows of a launch


@pytest.mark.parametrize("term", ["ssd", "lcc"])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_enough_samples_are_in_view_without_extrapolation(dim, term):
    make, lattices = (BL.ssd_problem, BL.SSD_LATTICES) if term == "ssd" else (BL.lcc_problem, BL.LCC_LATTICES)
    disp = make(dim, F32, 3, 0.4)[2]
    share = ssd_cpu.in_view(disp, lattices[dim][0])
    print("in view %s %d-D %s -> %s: %.3f" % (term, dim, *lattices[dim], share))
    assert disp.shape[0] == BL.B_LOOP and share >= 0.20, (term, dim, share)


def assert_distinct(want, bar, what):
    """every pair of the six items of `want` (6, ...) differs by more than 100 bars somewhere"""
    want = want.double().reshape(len(PINNED), -1)
    for i, j in itertools.combinations(range(len(PINNED)), 2):
        diff = float((want[i] - want[j]).abs().max())
        assert diff > 100 * bar, (what, PINNED[i], PINNED[j], diff, bar)


def pick(args):
    return [a[PINNED] if a is not None and a.shape[0] == BL.B_LOOP else a for a in args]


def case_ids(cases):
    return [c[0] for c in cases]


@pytest.mark.parametrize("case", BL.SSD_CASES, ids=case_ids(BL.SSD_CASES))
def test_pinned_items_of_ssd_differ(case):
    args, kw = BL.ssd_case(case)
    assert args[0].shape[0] == BL.B_LOOP and args[0].shape[1] == 2 and (args[1].shape[0] == BL.B_LOOP) == case[8]
    sg, sh = ssd_cpu.scales(*[args[i] for i in (0, 1, 3)])
    loss, g, h = ssd_cpu.reference(*pick(args), **dict(kw, hessian="full"))
    assert_distinct(loss, TOL32 * float(loss.abs().max()), ("ssd loss", case[0]))
    assert_distinct(g, TOL32 * (float(g.abs().max()) + sg), ("ssd gradient", case[0]))
    assert_distinct(h, TOL32 * (float(h.abs().max()) + sh), ("ssd hessian", case[0]))


@pytest.mark.parametrize("case", BL.LCC_CASES, ids=case_ids(BL.LCC_CASES))
def test_pinned_items_of_lcc_differ(case):
    args, kw = BL.lcc_case(case)
    assert args[0].shape[0] == BL.B_LOOP and args[0].shape[1] == 2
    loss, g, h, _ = lcc_cpu.truth(*pick(args), **dict(kw, hessian="full"))
    assert_distinct(loss, TOL32 * float(loss.abs().max()), ("lcc loss", case[0]))
    assert_distinct(g, 2 * TOL32 * float(g.abs().max()), ("lcc gradient", case[0]))
    assert_distinct(h, 2 * TOL32 * float(h.abs().max()), ("lcc hessian", case[0]))


def lcc_truth_at_a_stored_I(moving, fixed, disp, weight, window, eps, dtype, **kw):
    """`truth` of tests/test_lcc_cpu.py with I = pull(moving) rounded once to `dtype` before the window sums -- what csrc/lcc.hip
    stores between its first and its second kernel -- and everything else in float64.  -> (loss, gradient, diagonal of the Hessian)"""
    dim = disp.shape[-1]
    window = lcc_cpu.windows(window, dim)
    o = ssd_cpu.lattice(disp.shape[-dim - 1:-1], disp.dtype)
    x = (o + disp).double()
    d64 = x - o.double()
    J, w = fixed.double()[None], weight.double()
    I = interpol.grid_pull(moving.double(), d64, displacement=True, **kw).to(dtype).double()
    G = interpol.grid_grad(moving.double(), d64, displacement=True, **kw)
    wcc, cross, vJ, den, n, SI, SJ, wt = lcc_cpu.cc_terms(I, J, w, window, eps)
    a = wt * 2 * cross / den
    c = wt * 2 * cross * cross * vJ / (den * den)
    f = (a * SJ - c * SI) / n
    A, C, F = lcc_cpu.box(a, window), lcc_cpu.box(c, window), lcc_cpu.box(f, window)
    dI = -J * A + I * C + F
    return -wcc.flatten(1).sum(1), (dI.unsqueeze(-1) * G).sum(1), torch.stack([(C * G[..., d] * G[..., d]).sum(1) for d in range(dim)], -1)


@pytest.mark.parametrize("case", [c for c in BL.LCC_CASES if c[2] == "f32"], ids=case_ids([c for c in BL.LCC_CASES if c[2] == "f32"]))
def test_the_float32_storage_of_I_moves_the_lcc_truth_by_less_than_half_a_bar(case):
    """The condition behind the eps of the float32 cases (tests/batch_loops.py: LCC_CASES), from the truth alone: no kernel runs.
    Measured, worst of (loss, gradient, Hessian) over the whole batch in bars: at the eps of the case (1) 0.22, 0.06, 0.30, 0.10, 0.40
    for the five cases; at eps = 1e-5 the 1-D case stands at 39.9 and the 2-D window of 3 at 0.89."""
    args, kw = BL.lcc_case(case)
    kw = {k: v for k, v in kw.items() if k not in ("hessian", "window", "eps")}
    window, eps = case[7], case[10]
    dim = case[1]

    def moved(eps):
        want = lcc_cpu.truth(*args, window=window, eps=eps, hessian="diagonal", **kw)
        got = lcc_truth_at_a_stored_I(*args, window, eps, torch.float32, **kw)
        scale = lambda t: t.abs().flatten(1).max(1).values.reshape([-1] + [1] * (t.dim() - 1))
        r = [float(((g - w).abs() / (TOL32 * w.abs() + TOL32 * (scale(w) if w.dim() > 1 else 0.0)).clamp_min(1e-300)).max())
             for g, w in zip(got, want[:3])]
        return max(r)

    at_case = moved(eps)
    print("lcc %s: the float32 rounding of I moves the truth by %.3g bars at eps = %g" % (case[0], at_case, eps))
    assert at_case < 0.5, (case[0], at_case)
    if dim == 1:                                                        # ... and at the default eps it does not hold
        assert moved(1e-5) > 10.0


@pytest.mark.parametrize("case", BL.JACOBIAN_CASES, ids=case_ids(BL.JACOBIAN_CASES))
def test_pinned_items_of_jacobian_differ(case):
    name, shape, dt, order, bound = case
    u = BL.field(shape, BL.DT[dt], builder=jacobian_cpu)[PINNED]
    J = jacobian_cpu.oracle_jacobian(u, jacobian_cpu.BOUNDS.index(bound), order).double()
    det = jacobian_cpu.det_closed(J)
    assert_distinct(J, 2 * TOL32 * float(J.abs().max()), ("jacobian", name))
    assert_distinct(det, 2 * TOL32 * float(det.abs().max()), ("jacdet", name))


@pytest.mark.parametrize("case", BL.COMPOSE_CASES, ids=case_ids(BL.COMPOSE_CASES))
def test_pinned_items_of_compose_differ(case):
    name, (lshape, oshape), dt, order, bound, ex, lB = case
    left, right = BL.compose_fields(lshape, oshape, BL.DT[dt], lB=lB)
    assert left.shape[0] == (lB or BL.B_LOOP) and right.shape[0] == BL.B_LOOP
    assert torch.equal(right * 64, torch.round(right * 64))             # (dyadic: the coordinates are exact in float32)
    want = compose_cpu.composed((left if lB else left[PINNED]).double(), right[PINNED].double(), interpolation=order, bound=bound,
                                extrapolate=ex)
    assert_distinct(want, 2 * TOL32 * float(want.abs().max()), ("compose", name))
    if not ex:                                                          # in view: not `right` against `right`
        share = ssd_cpu.in_view(right, lshape)
        print("compose %s: %.3f of the samples in view" % (name, share))
        assert 0.20 <= share < 1.0, (name, share)


@pytest.mark.parametrize("case", BL.REG_CASES, ids=case_ids(BL.REG_CASES))
def test_pinned_items_of_the_regulariser_differ(case):
    name, shape, dt, bound, seed = case
    v = BL.field(shape, BL.DT[dt], seed=seed)[PINNED]
    S = reg_cpu.spatial_matrix(shape, bound, **BL.REG_WEIGHTS)
    Lv, E = reg_cpu.apply_dense(S, v), reg_cpu.energy_dense(S, v)
    assert_distinct(Lv, 2 * TOL32 * float(Lv.abs().max()), ("regulariser", name))
    assert_distinct(E, TOL32 * float(E.abs().max()), ("regulariser_energy", name))
    Sa = reg_cpu.spatial_matrix(shape, bound, absolute=BL.REG_ABSOLUTE, **BL.REG_WEIGHTS)
    Ea = reg_cpu.energy_dense(Sa, v)
    assert_distinct(Ea, TOL32 * float(Ea.abs().max()), ("regulariser_energy with absolute", name))
    # with absolute > 0 the energy of EVERY item is well away from zero (the condition of the relative bar of
    # tests/test_regulariser_gpu.py); without it the energy of a nearly constant field is not
    whole = BL.field(shape, BL.DT[dt], seed=seed)
    v2 = whole.double().square().reshape(BL.B_LOOP, -1).sum(1)
    assert bool((reg_cpu.energy_dense(Sa, whole) > 0.1 * v2).all())
    low = float((reg_cpu.energy_dense(S, whole) <= 0.1 * v2).double().mean())
    print("regulariser %s: %.4f of the items have an energy below 0.1 sum v^2 without `absolute`" % (name, low))
    assert low > 0 or len(shape) > 1                                    # (a lattice of four points: 0.4 % of the items)


@pytest.mark.parametrize("case", BL.SOLVE_CASES, ids=case_ids(BL.SOLVE_CASES))
def test_pinned_items_of_the_solver_differ(case):
    name, shape, dt, bound, kind = case
    sy = BL.solve_system(shape, bound, BL.SOLVE_WEIGHTS, 1., kind, BL.DT[dt])
    sub = dict(sy, g=sy["g"][PINNED], Hd=sy["Hd"][PINNED])
    x = BL.restated_batch(sub, 4)
    assert_distinct(x, 2 * TOL32 * float(x.abs().max()), ("regulariser_solve", name))
    # the tolerance of the early-stopping run stops some items before the cap and not others; the stopping test is
    # sigma <= tolerance^2 gamma after every iteration
    _, res = BL.restated_batch(sy, BL.EARLY_MAX_ITER - 1, history=True)
    stopped = float((res <= BL.EARLY_TOLERANCE).any(0).double().mean())
    print("solve %s: %.3f of the items stop before iteration %d" % (name, stopped, BL.EARLY_MAX_ITER))
    assert 0.15 < stopped < 0.85, (name, stopped)


def test_chunks_of_the_composed_form_is_the_composed_form_of_the_whole_batch():
    args = BL.ssd_problem(2, torch.float64, 3, 0.4)
    assert args[0].shape[0] == BL.B_LOOP and args[1].dim() == 3         # (fixed without a batch: handed to every chunk whole)
    fn = lambda m, f, u, w: interpol.ssd_gauss_newton(m, f, u, w, interpolation=3, bound="dct2", extrapolate=False, hessian="full")
    seen = []

    def spy(m, f, u, w):
        seen.append((m.shape[0], f.shape, u.shape[0], w.shape[0]))
        return fn(m, f, u, w)

    whole, parts = fn(*args), BL.chunks(spy, args)
    assert [s[0] for s in seen] == [32768, 32768, 2] and all(s[0] == s[2] == s[3] and s[1] == args[1].shape for s in seen)
    assert all(a.shape == b.shape and torch.equal(a, b) for a, b in zip(whole, parts))
    # a single tensor, an argument that is None, another chunk size
    one = BL.chunks(lambda m, f, u, w: fn(m, f, u, w)[1], list(args[:3]) + [None], size=30000)
    assert torch.equal(one, fn(*args[:3], None)[1])
    none = BL.chunks(lambda m, f, u, w: interpol.ssd_gauss_newton(m, f, u, w, hessian=None), args)
    assert none[2] is None and none[0].shape == (BL.B_LOOP,)


@pytest.mark.parametrize("kind", ["full", "diag", "none"])
def test_restated_batch_is_restated_item_by_item(kind):
    for dim in (1, 2, 3):
        shape = BL.SSD_LATTICES[dim][1]
        sy = BL.solve_system(shape, "dct2", st.ALL, 1., kind, torch.float64, B=7)
        got = BL.restated_batch(sy, 4)
        g = sy["g"].double()
        for b in range(7):
            want, its, _, _ = st.restated(sy["S"], sy["hh"], sy["Hd"][b], sy["c"], g[b].reshape(-1, dim), 4)
            assert its == 4
            assert float((got[b] - want).abs().max()) <= 1e-13 * float(want.abs().max()), (shape, kind, b)
