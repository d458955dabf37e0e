"""`interpol.regulariser_solve`: the algorithm, the composed form and the host layers (no GPU).

Truth everywhere -- here and in tests/test_regulariser_solve_gpu.py, which imports this module for it -- is never the code under
test.  The matrix is A = sum_d h_d^2 S (x) e_d e_d^T + blockdiag(H_o), with S the dense float64 spatial matrix of
tests/test_regulariser_cpu.py (`spatial_matrix`, built from the oracle's bound tables).  `restated` is the algorithm of the
issue for one batch item in float64, applying S and the per-voxel H densely; `dense_matrix` assembles A for
`torch.linalg.solve`.

The fixed inputs: g = field(shape, seed), B = 2; item 0 has the full symmetric Hessian H = 0.5 R R^T / D (R from randn), item 1
the diagonal one 0.2 rand.  One call takes one Hessian layout for the whole batch, so `hessian_arg` hands them over as
  'full' : K = D (D + 1) / 2, item 1 with zeros off the diagonal;
  'diag' : K = D, item 0 reduced to its diagonal (still positive semi-definite);
  'none' : no Hessian.
Without a Hessian and without `absolute`, L under dft / dct2 has the constants in its null space and the system is singular:
conjugate gradients on a singular system amplify rounding without bound, so no such case is compared against anything;
those weights are paired with a Hessian, or with bounds under which L is definite (zero, dst2, or a mix that has one).

Bars: float64 |got - want| <= 1e-11 |want| + 1e-11 max|want| (the project's); converged: 1e-11 max|want|.
"""
import math

import pytest
import torch

import interpol
import test_regulariser_cpu as truth

field = truth.field
TOL64 = 1e-11
VOXELS = truth.VOXELS
ALL = dict(absolute=0.3, membrane=0.7, bending=1.3)
_WANT = {}


def centre(vx, absolute=0., membrane=0., bending=0.):
    """c_d = h_d^2 [ absolute + membrane sum_e 2 / h_e^2 + bending ( sum_e 6 / h_e^4 + sum_{e != f} 4 / (h_e^2 h_f^2) ) ]"""
    a = [1.0 / (h * h) for h in vx]
    mixed = sum(4 * a[e] * a[f] for e in range(len(a)) for f in range(len(a)) if e != f)
    s = absolute + membrane * sum(2 * x for x in a) + bending * (sum(6 * x * x for x in a) + mixed)
    return torch.tensor([h * h * s for h in vx], dtype=torch.float64)


def voxels(dim, vx):
    return [float(vx)] * dim if not isinstance(vx, (list, tuple)) else [float(h) for h in vx]


def pack(Hm):
    """(..., D, D) symmetric -> (..., D (D + 1) / 2): the diagonal, then the upper triangle row by row"""
    dim = Hm.shape[-1]
    return torch.stack([Hm[..., d, d] for d in range(dim)] + [Hm[..., i, j] for i in range(dim) for j in range(i + 1, dim)], -1)


def unpack(h, dim):
    """the inverse of `pack`, and of the diagonal form: (..., K) -> (..., D, D)"""
    if h.shape[-1] == dim:
        return torch.diag_embed(h)
    Hm = torch.diag_embed(h[..., :dim])
    k = dim
    for i in range(dim):
        for j in range(i + 1, dim):
            Hm[..., i, j] = Hm[..., j, i] = h[..., k]
            k += 1
    return Hm


def fixed_hessians(shape, seed):
    """(2, *shape, D, D) float64: item 0 full, 0.5 R R^T / D; item 1 diagonal, 0.2 rand"""
    dim = len(shape)
    gen = torch.Generator().manual_seed(seed)
    R = torch.randn([*shape, dim, dim], generator=gen, dtype=torch.float64)
    d1 = 0.2 * torch.rand([*shape, dim], generator=gen, dtype=torch.float64)
    return torch.stack([0.5 * (R @ R.transpose(-1, -2)) / dim, torch.diag_embed(d1)])


def hessian_arg(shape, seed, kind, dtype=torch.float64):
    """the `hessian` argument ((2, *shape, K) in `dtype`, or None) and the matrices it stands for, (2, *shape, D, D) float64"""
    dim = len(shape)
    dense = fixed_hessians(shape, seed)
    if kind == "none":
        return None, torch.zeros_like(dense)
    arg = (pack(dense) if kind == "full" else torch.diagonal(dense, dim1=-2, dim2=-1).contiguous()).to(dtype)
    return arg, unpack(arg.double(), dim)


def restated(S, hh, Hd, c, g, max_iter, tolerance=0., keep=(), dtype=torch.float64):
    """The algorithm of `interpol.regulariser_solve` for ONE item: S (N, N), hh = h^2 (D), Hd (N, D, D), c (D), g (N, D) -> x (N, D),
    iterations, residual, and {k: x after min(k, iterations) iterations} for k in `keep`.  Fields in `dtype` (float64: the truth;
    float32: the reference's own rounding error, see FLOAT32_UNSTABLE_AT_24), inner products in double, alpha and beta rounded
    to `dtype` once."""
    S, hh, Hd, c, g = (t.to(dtype) for t in (S, hh, Hd, c, g))
    A = lambda v: (S @ v) * hh + torch.einsum("nde,ne->nd", Hd, v)
    M = Hd + torch.diag(c)
    Mi = lambda v: torch.linalg.solve(M, v[..., None])[..., 0]
    dot = lambda a, b: float((a.double() * b.double()).sum())
    x, r = torch.zeros_like(g), g.clone()
    z = Mi(r)
    p = z.clone()
    rho, gamma = dot(r, z), dot(g, g)
    its, sigma, kept = 0, 0.0, {}
    for _ in range(max_iter if gamma != 0 else 0):
        q = A(p)
        pi = dot(p, q)
        if pi <= 0 or rho <= 0:
            break
        alpha = torch.tensor(rho / pi, dtype=dtype)
        x, r = x + alpha * p, r - alpha * q
        z = Mi(r)
        rho1, sigma, its = dot(r, z), dot(r, r), its + 1
        if its in keep:
            kept[its] = x
        if sigma <= tolerance ** 2 * gamma:
            break
        p, rho = z + torch.tensor(rho1 / rho, dtype=dtype) * p, rho1
    return x, its, (math.sqrt(sigma / gamma) if its else 0.0), {k: kept.get(k, x) for k in keep}


def dense_matrix(S, hh, Hd):
    """A (N D x N D) = sum_d h_d^2 S (x) e_d e_d^T + blockdiag(H_o), unknowns ordered point by point"""
    N, D = Hd.shape[:2]
    A = torch.zeros(N, D, N, D, dtype=torch.float64)
    for d in range(D):
        A[:, d, :, d] += hh[d] * S
    n = torch.arange(N)
    A[n, :, n, :] += Hd
    return A.reshape(N * D, N * D)


def system(shape, seed, bound, w, vx, kind, dtype=torch.float64):
    """everything of one case: the arguments in `dtype` and the float64 pieces of the truth, as the device sees them (rounded)"""
    dim = len(shape)
    g = field(shape, seed, dtype)
    h, Hd = hessian_arg(shape, seed + 1000, kind, dtype)
    S = truth.spatial_matrix(shape, bound, voxel_size=vx, **w)
    return dict(g=g, h=h, S=S, hh=truth.h2(dim, vx), Hd=Hd.reshape(2, -1, dim, dim), c=centre(voxels(dim, vx), **w),
                kw=dict(voxel_size=vx, bound=bound, **w))


def want_after(key, sy, keep, dtype=torch.float64):
    """{k: (2, *shape, D)} after k iterations, computed once per case (`key`) and shared"""
    key = (key, dtype)
    if key not in _WANT:
        g = sy["g"].double()
        per = [restated(sy["S"], sy["hh"], sy["Hd"][b], sy["c"], g[b].reshape(-1, g.shape[-1]), max(keep), keep=keep, dtype=dtype)[3]
               for b in range(2)]
        _WANT[key] = {k: torch.stack([per[b][k] for b in range(2)]).reshape(g.shape) for k in keep}
    return _WANT[key]


def close(got, want, tol):
    """error / bar of |got - want| <= tol |want| + tol max|want|, the worst element"""
    got = got.detach().cpu().double()
    assert got.shape == want.shape and bool(torch.isfinite(got).all())
    return float(((got - want).abs() / (tol * want.abs() + tol * float(want.abs().max()))).max())


def cases_for(dim):
    """(weights, bound, voxel size, Hessian kind): in 3-D every one of the 7 weight modes, in 1-D and 2-D membrane, bending
    and all three; the four symmetric bounds and one per-dimension mix; the Hessian none, diagonal and full; one anisotropic
    voxel size.  No singular system (see the header), and none that is badly conditioned: rounding moves the iterates of
    conjugate gradients by about cond(A) times the unit roundoff, so a float32 run can follow the float64 truth to the 1e-5
    bar only while cond(A) 2^-24 is well below it.  Every case keeps cond(A) below about 2e3 a priori (the converged cases
    of the issue have 56 to 453; the one it names for the fixed counts alone, dct2 with all three terms and anisotropic voxels,
    has 1027 / 3780 at (5, 4, 23) and is the worst here): `absolute` = a bounds it by (a + ||L||) / a -- ||L|| = 4 membrane sum_e 1 / h_e^2 + 16 bending
    (sum_e 1 / h_e^2)^2, 12 and 144 in 3-D with unit voxels; or the Hessian does (0.2 rand and 0.5 R R^T / D have eigenvalues of
    order 0.1); or, without either, the zero / dst2 bounds do on the short extents of the 3-D shapes (membrane: the smallest
    eigenvalue is sum_e (pi / (n_e + 1))^2 over the zero-bound dimensions, 0.07 and more for n <= 9).  In 1-D, (130,) under
    'zero' without a Hessian has cond(A) of about 6e4 and is not used."""
    mix = ["zero", "dft", "dst2"][:dim]
    if dim == 3:
        return [(dict(absolute=2.0), "dft", 1., "full"), (dict(membrane=1.0), "dft", 1., "diag"),
                (dict(absolute=0.1, membrane=1.0), "dct2", 1., "none"), (dict(bending=1.0), "dct2", 1., "full"),
                (dict(absolute=0.5, bending=1.0), "dft", 1., "none"), (dict(membrane=0.7, bending=0.3), mix, 1., "none"),
                (ALL, "dct2", VOXELS[3], "full"), (dict(membrane=1.0), "zero", 1., "none"), (dict(bending=1.0), "dst2", 1., "diag")]
    return [(dict(membrane=1.0), "dft", 1., "diag"), (dict(bending=1.0), "dct2", 1., "full"), (ALL, "dst2", VOXELS[dim], "none"),
            (dict(membrane=0.7, bending=1.3), "zero", 1., "diag"), (ALL, mix, 1., "full")]


# (shape, index into cases_for(3)): systems on which conjugate gradients in float32 leave the float64 iterates between 8 and 24
# iterations whoever runs them.  `restated` itself, run in float32 on the dense matrix, is 5.5, 209 and 1.05 float32 bars from
# its float64 run after 24 iterations there, and at most 0.27 after 8 (test_float32_reference_run_on_the_unstable_systems
# asserts both); on every other (shape, case) of the device test it stays below 0.5 bars at 1, 8 and 24 iterations.  The
# spectra of these three come in a few tight clusters ((5, 4, 23) dft without a Hessian: exactly repeated eigenvalues; the
# 2-ring on extents of 3 and 4): once the clusters are resolved the next search direction is made of rounding errors, and
# when that happens depends on the precision.  The device test compares them in float64 at every count and in float32 at 1
# and 8 iterations; both precisions still converge to the dense solution (the converged test has (3, 3, 3)).
FLOAT32_UNSTABLE_AT_24 = {((5, 4, 23), 4), ((3, 3, 3), 3), ((4, 2, 5), 5)}
# ... and the one of them that is not reproducible after 24 iterations in float64 either: (3, 3, 3), bending alone under dct2
# (81 unknowns, the eigenvalues of L are the squares of 0, 1, ..., 7, 9).  Scaling every g by 1 + 2^-52 randn moves the float64
# reference run by hundreds of float64 bars after 24 iterations (363 with the seed of the test, which asserts it) and by 0.001
# after 8; such a perturbation moves (5, 4, 23) case 4 and (4, 2, 5) case 5 by about 0.02 bars, every other case by 0.0006 at most.
FLOAT64_UNSTABLE_AT_24 = {((3, 3, 3), 3)}



def float32_floor_above_the_bar(shape, n):
    """Case 3 of cases_for(3) -- bending alone under dct2, full Hessian -- on a shape with an extent of 1 or 2.  Along such a
    dimension every tap of the 2-ring folds onto the same one or two points and the coefficients cancel: L vanishes there, but a
    float32 stencil still rounds each of the 25 products, an absolute error of 2^-24 144 max|p| per application of L (144: the
    |coefficients| of a row, `taps_abs_sum`), while the smallest eigenvalue of A is the Hessian's alone, of order 0.1.  The
    solution is therefore only good to 2^-24 144 / 0.1 = 9e-5 of its size, above the 1e-5 bar, whatever the iteration does (the
    dense reference has the cancelled entries exactly and does not see this; the fused kernels are 1.7 bars off at (2, 1, 1)
    after 8 iterations, the composed form in float32 on the host 0.18).  These are compared in float64 only.  With `absolute` or
    `membrane` in L, or under dst2 (which does not cancel), the smallest eigenvalue is not left to the Hessian."""
    return n == 3 and len(shape) == 3 and min(shape) <= 2


# the cases of the converged comparison: shape, bound, weights, voxel size
CONVERGED = [((130,), "dct2", dict(absolute=0.01, membrane=0.7, bending=1.3), 1.),
             ((19, 11), "dft", dict(membrane=1.0), [0.5, 1.25]),
             ((5, 4, 23), ["zero", "dft", "dst2"], dict(membrane=0.7, bending=0.3), 1.),
             ((3, 3, 3), "dft", dict(absolute=0.1, bending=1.0), 1.),
             ((1, 2, 3), "dct2", dict(absolute=0.1, membrane=1.0, bending=1.0), 1.)]
CONVERGED_IDS = ["x".join(map(str, c[0])) for c in CONVERGED]


def converged_truth(case, dtype=torch.float64):
    """the system of one converged case, its dense solution (2, *shape, D) and cond(A) per item; A is checked to be symmetric
    positive definite"""
    shape, bound, w, vx = CONVERGED[case]
    sy = system(shape, 700 + case, bound, w, vx, "full", dtype)
    g = sy["g"].double()
    want, cond = [], []
    for b in range(2):
        A = dense_matrix(sy["S"], sy["hh"], sy["Hd"][b])
        assert float((A - A.T).abs().max()) <= 1e-13 * float(A.abs().max())
        ev = torch.linalg.eigvalsh(0.5 * (A + A.T))
        assert float(ev[0]) > 0
        cond.append(float(ev[-1] / ev[0]))
        want.append(torch.linalg.solve(A, g[b].reshape(-1)).reshape(g[b].shape))
    return sy, torch.stack(want), cond


# ---------------------------------------------------------------------------------------------------------------------
# 1. fixed iteration counts against the restated algorithm
# ---------------------------------------------------------------------------------------------------------------------
FIXED_SHAPES = [(130,), (19, 11), (5, 4, 23), (1, 2, 3), (2, 1, 1)]


@pytest.mark.parametrize("shape", FIXED_SHAPES, ids=["x".join(map(str, s)) for s in FIXED_SHAPES])
def test_fixed_iteration_counts_match_the_restated_algorithm(shape):
    dim = len(shape)
    worst = 0.0
    for n, (w, bound, vx, kind) in enumerate(cases_for(dim)):
        sy = system(shape, 600 + n, bound, w, vx, kind)
        want = want_after(("cpu", shape, n), sy, (1, 8, 24))
        for k in (1, 8, 24):
            got, info = interpol.regulariser_solve(sy["g"], sy["h"], max_iter=k, tolerance=0., return_info=True, **sy["kw"])
            assert got.dtype == torch.float64 and got.shape == sy["g"].shape
            assert info.iterations.dtype == torch.int64 and info.residual.dtype == torch.float64
            assert info.iterations.shape == (2,) and info.residual.shape == (2,) and bool((info.iterations <= k).all())
            ratio = close(got, want[k], TOL64)
            worst = max(worst, ratio)
            assert ratio <= 1.0, (shape, w, bound, vx, kind, k, ratio)
    print("fixed counts %s: worst error / bar = %.3g" % (shape, worst))


def test_float32_reference_run_on_the_unstable_systems():
    """the reason for FLOAT32_UNSTABLE_AT_24, from the reference alone: its float32 run against its float64 run"""
    order = [(130,), (19, 11), (9, 5, 67), (5, 4, 23), (3, 3, 3), (1, 2, 3), (2, 1, 1), (4, 2, 5)]      # (the seeds of the device test)
    for shape, n in sorted(FLOAT32_UNSTABLE_AT_24):
        w, bound, vx, kind = cases_for(3)[n]
        sy = system(shape, 100 * order.index(shape) + n, bound, w, vx, kind, torch.float32)
        want = want_after(("unstable", shape, n), sy, (8, 24))
        ref32 = want_after(("unstable", shape, n), sy, (8, 24), torch.float32)
        at8, at24 = close(ref32[8], want[8], 1e-5), close(ref32[24], want[24], 1e-5)
        print("float32 reference run %s case %d: error / bar = %.3g after 8 iterations, %.3g after 24" % (shape, n, at8, at24))
        assert at8 <= 0.5 and at24 > 1.0, (shape, n, at8, at24)
        if (shape, n) in FLOAT64_UNSTABLE_AT_24:
            gen = torch.Generator().manual_seed(0)
            moved = dict(sy, g=sy["g"].double() * (1 + 2.0 ** -52 * torch.randn(sy["g"].shape, generator=gen, dtype=torch.float64)))
            pert = want_after(("unstable-moved", shape, n), moved, (8, 24))
            at8, at24 = close(pert[8], want[8], TOL64), close(pert[24], want[24], TOL64)
            print("float64 reference run, g moved by an ulp: error / bar = %.3g after 8 iterations, %.3g after 24" % (at8, at24))
            assert at8 <= 0.1 and at24 > 1.0, (shape, n, at8, at24)


def test_the_hard_system_at_fixed_counts():
    """(5, 4, 23) dct2 with all three terms and anisotropic voxels (cond about 1e3: far from converged after 24 iterations)"""
    shape = (5, 4, 23)
    sy = system(shape, 650, "dct2", ALL, VOXELS[3], "full")
    want = want_after(("cpu-hard", shape), sy, (1, 8, 24))
    for k in (1, 8, 24):
        got = interpol.regulariser_solve(sy["g"], sy["h"], max_iter=k, **sy["kw"])
        assert close(got, want[k], TOL64) <= 1.0, k


# ---------------------------------------------------------------------------------------------------------------------
# 2. converged against the dense solve
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(CONVERGED)), ids=CONVERGED_IDS)
def test_converged_solution_is_the_dense_solve(case):
    sy, want, cond = converged_truth(case)
    got, info = interpol.regulariser_solve(sy["g"], sy["h"], max_iter=200, return_info=True, **sy["kw"])
    err = float((got - want).abs().max()) / float(want.abs().max())
    print("converged %s: cond(A) = %.0f / %.0f, error / max|want| = %.3g, iterations %s" % (CONVERGED[case][0], cond[0], cond[1], err, info.iterations.tolist()))
    assert err <= TOL64, err


# ---------------------------------------------------------------------------------------------------------------------
# 3. stopping
# ---------------------------------------------------------------------------------------------------------------------
def check_stopping(dev, dtype=torch.float64):
    """shared with the device test: the assertions of the issue's stopping test on `dev`"""
    shape = (5, 4, 23)
    sy = system(shape, 800, ["zero", "dft", "dst2"], dict(membrane=0.7, bending=0.3), 1., "full", dtype)
    g, h = sy["g"].to(dev), sy["h"].to(dev)
    x, info = interpol.regulariser_solve(g, h, max_iter=200, tolerance=1e-3, return_info=True, **sy["kw"])
    its = info.iterations.tolist()
    assert all(0 < i < 200 for i in its) and bool((info.residual <= 1e-3).all()) and bool((info.residual > 0).all()), (its, info.residual)
    for b in range(2):
        again, inf2 = interpol.regulariser_solve(g, h, max_iter=its[b], tolerance=0., return_info=True, **sy["kw"])
        assert torch.equal(again[b], x[b]) and int(inf2.iterations[b]) == its[b], b
        assert float(inf2.residual[b]) == float(info.residual[b]), b
    # an item with g = 0 next to a non-zero one
    g0 = g.clone()
    g0[0] = 0
    x0, info0 = interpol.regulariser_solve(g0, h, max_iter=200, tolerance=1e-3, return_info=True, **sy["kw"])
    assert not bool(x0[0].any()) and int(info0.iterations[0]) == 0 and float(info0.residual[0]) == 0.0
    assert bool(torch.isfinite(x0).all()) and bool(torch.isfinite(info0.residual).all())
    assert torch.equal(x0[1], x[1]) and int(info0.iterations[1]) == its[1] and float(info0.residual[1]) == float(info.residual[1])
    # max_iter = 0
    z, infz = interpol.regulariser_solve(g, h, max_iter=0, return_info=True, **sy["kw"])
    assert z.shape == g.shape and z.dtype == g.dtype and not bool(z.any())
    assert not bool(infz.iterations.any()) and not bool(infz.residual.any())
    assert x.device == g.device and info.iterations.device == g.device and info.residual.device == g.device


def test_stopping():
    check_stopping("cpu")


# ---------------------------------------------------------------------------------------------------------------------
# 4. arguments
# ---------------------------------------------------------------------------------------------------------------------
def test_arguments():
    shape = (4, 3, 5)
    g = field(shape, 900)
    h, _ = hessian_arg(shape, 901, "full")
    ok = dict(membrane=1.0, bound="dct2", max_iter=4)
    for bad in ("replicate", "dct1", "dst1"):
        with pytest.raises(ValueError):
            interpol.regulariser_solve(g, h, **dict(ok, bound=bad))
        with pytest.raises(ValueError):
            interpol.regulariser_solve(g, h, **dict(ok, bound=["dct2", bad, "dft"]))
    for K in (1, 2, 4, 5, 9):
        with pytest.raises(ValueError):
            interpol.regulariser_solve(g, torch.ones(2, *shape, K, dtype=torch.float64), **ok)
    with pytest.raises(ValueError):
        interpol.regulariser_solve(g, h, bound="dct2", max_iter=4)                       # all weights zero
    with pytest.raises(ValueError):
        interpol.regulariser_solve(g, h, **dict(ok, max_iter=-1))
    with pytest.raises(ValueError):
        interpol.regulariser_solve(g, h, tolerance=-1e-3, **ok)
    with pytest.raises(TypeError):
        interpol.regulariser_solve(g, h, membrane=torch.tensor(1.0), bound="dct2")
    for t in (g, h):
        t.requires_grad_()
        with pytest.raises(RuntimeError, match="not differentiable"):
            interpol.regulariser_solve(g, h, **ok)
        with torch.no_grad():
            x = interpol.regulariser_solve(g, h, **ok)
        assert not x.requires_grad and bool(torch.isfinite(x).all())
        t.requires_grad_(False)


def test_batch_broadcasting():
    shape = (4, 3, 5)
    g = field(shape, 910)
    h, _ = hessian_arg(shape, 911, "full")
    kw = dict(absolute=0.1, membrane=1.0, bound="dft", max_iter=6)
    x, info = interpol.regulariser_solve(g, h[0], return_info=True, **kw)
    xe, infe = interpol.regulariser_solve(g, h[:1].expand(2, *h.shape[1:]), return_info=True, **kw)
    assert torch.equal(x, xe) and torch.equal(info.iterations, infe.iterations) and torch.equal(info.residual, infe.residual)
    # leading batch dimensions fold, and an unbatched gradient takes the batch of the Hessian
    x2 = interpol.regulariser_solve(g.reshape(2, 1, *g.shape[1:]), h[0], **kw)
    assert x2.shape == (2, 1, *g.shape[1:]) and torch.equal(x2.reshape(x.shape), x)
    x3, inf3 = interpol.regulariser_solve(g[0], h, return_info=True, **kw)
    assert x3.shape == g.shape and inf3.iterations.shape == (2,)
    assert torch.equal(x3[0], x[0])
    x4, inf4 = interpol.regulariser_solve(g[0], h[0], return_info=True, **kw)
    assert x4.shape == g[0].shape and inf4.iterations.shape == () and torch.equal(x4, x[0])


def test_bf16_returns_bf16():
    shape = (5, 4, 23)
    g = field(shape, 920, torch.bfloat16)
    h, _ = hessian_arg(shape, 921, "full", torch.bfloat16)
    kw = dict(membrane=0.7, bending=0.3, bound=["zero", "dft", "dst2"], max_iter=24)
    x = interpol.regulariser_solve(g, h, **kw)
    assert x.dtype == torch.bfloat16
    ref = interpol.regulariser_solve(g.float(), h.float(), **kw)
    assert ref.dtype == torch.float32
    assert float((x.float() - ref).abs().max()) <= 1e-2 * float(ref.abs().max())


def test_four_dimensions_take_the_composed_form():
    shape = (3, 2, 4, 3)
    g = field(shape, 930)
    h, Hd = hessian_arg(shape, 931, "full")
    w = dict(absolute=0.1, membrane=1.0)
    S = truth.spatial_matrix(shape, "dft", **w)
    got = interpol.regulariser_solve(g, h, bound="dft", max_iter=200, **w)
    for b in range(2):
        A = dense_matrix(S, truth.h2(4), Hd[b].reshape(-1, 4, 4))
        want = torch.linalg.solve(A, g[b].reshape(-1)).reshape(g[b].shape)
        assert float((got[b] - want).abs().max()) <= TOL64 * float(want.abs().max())
