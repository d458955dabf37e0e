"""The linear-elastic terms of `interpol.regulariser` / `regulariser_energy` / `regulariser_solve` (`shears`, `div`) and the
'sliding' bound: the definition, the composed form and the host layers (no GPU).

Truth everywhere -- here and in tests/test_elastic_gpu.py, which imports this module for it -- is the float64 matrix of the FULL
operator on (N x D) values, row and column (o, c) at o D + c:

    (L v)_c = h_c^2 [ absolute v_c + (membrane + shears) sum_e A_e v_c + (shears + div) A_c v_c
                      + bending ( sum_e B_e v_c + sum_{e != f} A_e A_f v_c ) ]  -  (shears + div) sum_{e != c} X_ce v_e
    X_ce = C_c (x) C_e,   C f [o] = (f~[o + 1] - f~[o - 1]) / 2

assembled in `entries` from 1-D tap tables (A = (-1, 2, -1) / h^2, B = (1, -4, 6, -4, 1) / h^4, C = (-1, 0, 1) / 2), each built row
by row from `oracle.bound_index` / `oracle.bound_sign` under the bound OF THE COMPONENT it acts on, and Kronecker products.
`component_bound`: in a 'sliding' dimension d component d has 'dst2' and every other one 'dct2'.  The entries are kept as
(row, column, value) so that the large shapes of the GPU module stay cheap; `dense` sums them into the matrix.  Never the code
under test.

Bar of the float64 comparisons (that of tests/test_regulariser_cpu.py): |got - want| <= 1e-11 |want| + 1e-11 max|want|.
"""
import itertools
import math

import numpy
import pytest
import torch

import interpol
from interpol import torch_kernels
from oracle import oracle
from test_regulariser_cpu import field, assert_close

NAMES = ["zero", "replicate", "dct1", "dct2", "dst1", "dst2", "dft"]
TAPS_A = {0: 2.0, -1: -1.0, 1: -1.0}
TAPS_B = {0: 6.0, -1: -4.0, 1: -4.0, -2: 1.0, 2: 1.0}
TAPS_C = {-1: -0.5, 1: 0.5}
VOXELS = {1: [1.5], 2: [0.5, 1.25], 3: [2.0, 0.75, 1.5], 4: [1.0, 0.5, 1.25, 2.0]}
ELASTIC = dict(shears=0.6, div=0.9)
FIVE = dict(absolute=0.3, membrane=0.7, bending=1.3, shears=0.6, div=0.9)
# elastic alone, everything together, the three old terms (under sliding too), shears alone, div + membrane
WEIGHTS = [ELASTIC, FIVE, dict(absolute=0.3, membrane=0.7, bending=1.3), dict(shears=1.0), dict(membrane=0.5, div=2.0)]
SYM_SHAPES = [(1,), (2,), (5,), (1, 1), (2, 1), (1, 2), (2, 3), (4, 5), (1, 1, 1), (2, 1, 1), (1, 2, 3), (3, 3, 3), (4, 2, 5)]
_CACHE = {}


def ids(shapes):
    return ["x".join(map(str, s)) for s in shapes]


def component_bound(bound, c, e):
    """the bound of component c along dimension e"""
    if bound[e] == "sliding":
        return "dst2" if c == e else "dct2"
    return bound[e]


def stencil_matrix(n, bound, taps):
    """(n x n) float64: row o holds sum_t taps[t] f~[o + t], f~[i] = sign(i) f[index(i)] by the oracle's tables"""
    code = NAMES.index(bound)
    M = torch.zeros(n, n, dtype=torch.float64)
    for o in range(n):
        for t, c in taps.items():
            s = oracle.bound_sign(code, o + t, n)
            M[o, oracle.bound_index(code, o + t, n)] += c * (1 if s is None else s)
    return M


def kron_entries(mats, shape):
    """(row, column, value) of the Kronecker product of one matrix per dimension (None: the identity), row-major.  Zeros of
    the factors are kept out; entries that meet at one place are NOT merged (the caller sums them)."""
    row = col = torch.zeros(1, dtype=torch.int64)
    val = torch.ones(1, dtype=torch.float64)
    for m, n in zip(mats, shape):
        if m is None:
            i = j = torch.arange(n)
            w = torch.ones(n, dtype=torch.float64)
        else:
            i, j = m.nonzero(as_tuple=True)
            w = m[i, j]
        row = (row[:, None] * n + i[None, :]).reshape(-1)
        col = (col[:, None] * n + j[None, :]).reshape(-1)
        val = (val[:, None] * w[None, :]).reshape(-1)
    return row, col, val


def as_list(x, dim):
    return [x] * dim if not isinstance(x, (list, tuple)) else list(x)


def entries(shape, bound, voxel_size=1., absolute=0., membrane=0., bending=0., shears=0., div=0.):
    """(row, column, value, N D) of L; bound: a name or one per dim ('sliding' among them); voxel_size: a number or one per dim"""
    dim = len(shape)
    bound = as_list(bound, dim)
    vx = [float(h) for h in as_list(voxel_size, dim)]
    key = (tuple(shape), tuple(bound), tuple(vx), absolute, membrane, bending, shears, div)
    if key in _CACHE:
        return _CACHE[key]
    N = math.prod(shape)
    rows, cols, vals = [], [], []

    def add(c, e, mats, scale):
        """block (c, e) += scale * kron(mats)"""
        if scale == 0:
            return
        r, k, v = kron_entries(mats, shape)
        rows.append(r * dim + c)
        cols.append(k * dim + e)
        vals.append(v * scale)

    for c in range(dim):
        h2 = vx[c] ** 2
        A = [stencil_matrix(shape[e], component_bound(bound, c, e), TAPS_A) / vx[e] ** 2 for e in range(dim)]
        B = [stencil_matrix(shape[e], component_bound(bound, c, e), TAPS_B) / vx[e] ** 4 for e in range(dim)]
        add(c, c, [None] * dim, h2 * absolute)
        for e in range(dim):
            one = [None] * dim
            one[e] = A[e]
            add(c, c, one, h2 * (membrane + shears + (shears + div if e == c else 0.)))
            one[e] = B[e]
            add(c, c, one, h2 * bending)
            for f in range(dim):
                if f != e:
                    two = [None] * dim
                    two[e], two[f] = A[e], A[f]
                    add(c, c, two, h2 * bending)
        for e in range(dim):
            if e != c:
                # X_ce acts on component e, extended by the bounds of component e
                two = [None] * dim
                two[c] = stencil_matrix(shape[c], component_bound(bound, e, c), TAPS_C)
                two[e] = stencil_matrix(shape[e], component_bound(bound, e, e), TAPS_C)
                add(c, e, two, -(shears + div))
    out = (torch.cat(rows), torch.cat(cols), torch.cat(vals), N * dim)
    while len(_CACHE) >= 16:
        _CACHE.pop(next(iter(_CACHE)))
    _CACHE[key] = out
    return out


def dense(E):
    row, col, val, n = E
    return torch.zeros(n * n, dtype=torch.float64).index_add_(0, row * n + col, val).reshape(n, n)


def apply_entries(E, v, transpose=False):
    """L v (or L^T v) in float64: v (B, *shape, D) -> the same shape"""
    row, col, val, n = E
    if transpose:
        row, col = col, row
    flat = v.double().reshape(v.shape[0], n)
    out = torch.zeros_like(flat)
    out.index_add_(1, row, flat[:, col] * val)
    return out.reshape(v.shape)


def energy_entries(E, v):
    return 0.5 * (v.double() * apply_entries(E, v)).reshape(v.shape[0], -1).sum(1)


def norm_inf(E):
    """an upper bound of ||L||_inf: the sum of the absolute entries of a row BEFORE entries that fold onto one place are merged --
    the size of the terms that cancel where they do"""
    row, _, val, n = E
    return float(torch.zeros(n, dtype=torch.float64).index_add_(0, row, val.abs()).max())


def bound_mixes(dim, names=("zero", "dft", "sliding")):
    return [list(b) for b in itertools.product(names, repeat=dim)]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the definition: symmetry, definiteness, the symbol, the null space
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SYM_SHAPES, ids=ids(SYM_SHAPES))
def test_L_is_symmetric_psd_under_zero_dft_sliding(shape):
    dim = len(shape)
    for bound in bound_mixes(dim):
        for w in WEIGHTS:
            L = dense(entries(shape, bound, VOXELS[dim], **w))
            assert float((L - L.T).abs().max()) == 0.0, (shape, bound, w)
            assert float(torch.linalg.eigvalsh(L).min()) >= -1e-12 * float(L.abs().max()), (shape, bound, w)


def test_L_is_not_symmetric_for_one_reflecting_bound_per_dimension():
    for bound in ("dct2", "dst2", "replicate", "dct1", "dst1"):
        L = dense(entries((4, 5), bound, 1., shears=1.0, div=1.0))
        assert float((L - L.T).abs().max()) >= 0.5, bound
    # ... while the three old terms are, under dct2 / dst2, as they were
    for bound in ("dct2", "dst2"):
        L = dense(entries((4, 5), bound, 1., absolute=1.0, membrane=1.0, bending=1.0))
        assert float((L - L.T).abs().max()) == 0.0, bound


@pytest.mark.parametrize("shape", [(8,), (6, 5), (4, 5, 6)], ids=["1d", "2d", "3d"])
def test_plane_waves_meet_the_symbol(shape):
    """dft: L (p e^{i theta.o}) = diag(h) [ shears (|s|^2 I + N) + div N ] diag(h) p e^{i theta.o},
    N = diag(s_c^2) + offdiag(t_c t_e), s = 2 sin(theta / 2) / h, t = sin(theta) / h"""
    dim = len(shape)
    vx = torch.tensor(VOXELS[dim], dtype=torch.float64)
    E = entries(shape, "dft", VOXELS[dim], **ELASTIC)
    mu, lam = ELASTIC["shears"], ELASTIC["div"]
    grid = torch.stack(torch.meshgrid(*[torch.arange(n, dtype=torch.float64) for n in shape], indexing="ij"), -1)
    p = torch.tensor([0.7, -1.1, 0.4], dtype=torch.float64)[:dim]
    for k in itertools.product(*[range(0, n, max(1, n // 3)) for n in shape]):
        theta = torch.tensor([2 * math.pi * ki / n for ki, n in zip(k, shape)], dtype=torch.float64)
        s, t = 2 * torch.sin(theta / 2) / vx, torch.sin(theta) / vx
        Nm = torch.outer(t, t)
        Nm[range(dim), range(dim)] = s * s
        symbol = vx[:, None] * (mu * (float((s * s).sum()) * torch.eye(dim, dtype=torch.float64) + Nm) + lam * Nm) * vx[None, :]
        phase = (grid * theta).sum(-1)
        for wave in (torch.cos(phase), torch.sin(phase)):
            v = (wave[..., None] * p)[None]
            want = (wave[..., None] * (symbol @ p))[None]
            got = apply_entries(E, v)
            assert float((got - want).abs().max()) <= 1e-12 * (1 + float(want.abs().max())), (shape, k)
            assert_close(interpol.regulariser(v, voxel_size=VOXELS[dim], bound="dft", **ELASTIC), got, 1e-11, (shape, k),
                         cancelled=norm_inf(E))


@pytest.mark.parametrize("shape", [(9,), (7, 8), (6, 7, 8)], ids=["1d", "2d", "3d"])
def test_affine_fields_are_in_the_interior_null_space(shape):
    dim = len(shape)
    gen = torch.Generator().manual_seed(5)
    M = torch.randn(dim, dim, generator=gen, dtype=torch.float64)
    grid = torch.stack(torch.meshgrid(*[torch.arange(n, dtype=torch.float64) for n in shape], indexing="ij"), -1)
    v = (grid @ M.T + torch.randn(dim, generator=gen, dtype=torch.float64))[None]
    for w, ring in ((ELASTIC, 1), (dict(membrane=0.7, **ELASTIC), 1), (dict(membrane=0.7, bending=1.3, **ELASTIC), 2)):
        for bound in ("zero", "sliding", "dct2"):
            E = entries(shape, bound, VOXELS[dim], **w)
            inner = tuple([slice(None)] + [slice(ring, n - ring) for n in shape])
            bar = 1e-12 * norm_inf(E) * float(v.abs().max())
            assert float(apply_entries(E, v)[inner].abs().max()) <= bar, (shape, w, bound)
            assert float(interpol.regulariser(v, voxel_size=VOXELS[dim], bound=bound, **w)[inner].abs().max()) <= bar, (shape, w, bound)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the composed form is the dense matrix
# ---------------------------------------------------------------------------------------------------------------------
COMPOSED_SHAPES = [(7,), (5, 4), (3, 4, 5), (1,), (2,), (1, 2, 3), (1, 3), (2, 2, 3, 2)]


@pytest.mark.parametrize("shape", COMPOSED_SHAPES, ids=ids(COMPOSED_SHAPES))
def test_composed_form_matches_the_dense_matrix(shape):
    dim = len(shape)
    v = field(shape, 40 + dim)
    bounds = NAMES + ["sliding", (["sliding", "zero", "dft", "dct2"] * 2)[:dim], (["dst1", "sliding", "sliding", "replicate"])[:dim]]
    for bound in bounds:
        for w in WEIGHTS:
            for vx in (1., VOXELS[dim]):
                E = entries(shape, bound, vx, **w)
                what = (shape, bound, w, vx)
                cancelled = norm_inf(E) * float(v.abs().max())
                got = interpol.regulariser(v, voxel_size=vx, bound=bound, **w)
                assert got.dtype == v.dtype and got.shape == v.shape
                assert_close(got, apply_entries(E, v), 1e-11, what, cancelled=cancelled)
                En = interpol.regulariser_energy(v, voxel_size=vx, bound=bound, **w)
                scale = 0.5 * cancelled * v.abs().reshape(2, -1).sum(1)
                assert bool(((En.double() - energy_entries(E, v)).abs() <= 1e-11 * scale).all()), what


@pytest.mark.parametrize("bound", ["dft", "sliding", ["zero", "sliding"], "dct2", "replicate"], ids=str)
def test_gradients_are_the_transposed_matrix(bound):
    """autograd.grad: L^T g for the matvec, 0.5 (L + L^T) v for the energy -- dct2 and replicate are not symmetric here"""
    shape, vx = (4, 5), VOXELS[2]
    E = entries(shape, bound, vx, **FIVE)
    v = field(shape, 61).requires_grad_()
    g = field(shape, 62)
    got, = torch.autograd.grad(interpol.regulariser(v, voxel_size=vx, bound=bound, **FIVE), v, g)
    assert_close(got, apply_entries(E, g, transpose=True), 1e-11, ("matvec", bound))
    gE = torch.tensor([0.7, -1.3], dtype=torch.float64)
    got, = torch.autograd.grad(interpol.regulariser_energy(v, voxel_size=vx, bound=bound, **FIVE), v, gE)
    vd = v.detach()
    want = 0.5 * (apply_entries(E, vd) + apply_entries(E, vd, transpose=True)) * gE.reshape(2, 1, 1, 1)
    assert_close(got, want, 1e-11, ("energy", bound))
    sym = float((dense(E) - dense(E).T).abs().max()) == 0.0
    assert sym == (bound not in ("dct2", "replicate"))
    assert interpol.autograd._regulariser_symmetric(interpol.autograd.regulariser_bound_codes(bound, 2), tuple(FIVE.values())) == sym


def test_gradcheck_through_the_elastic_terms():
    v = field((3, 4), 63, B=1).requires_grad_()
    for bound in ("sliding", "dct2"):
        assert torch.autograd.gradcheck(lambda x: interpol.regulariser(x, voxel_size=VOXELS[2], bound=bound, **FIVE), (v,))
        assert torch.autograd.gradcheck(lambda x: interpol.regulariser_energy(x, voxel_size=VOXELS[2], bound=bound, **FIVE), (v,))


# ---------------------------------------------------------------------------------------------------------------------
# 3. the solve
# ---------------------------------------------------------------------------------------------------------------------
def full_hessian(shape, seed):
    """(1, *shape, K) symmetric positive definite, the diagonal first, then the upper triangle row by row -- and its matrix"""
    dim = len(shape)
    gen = torch.Generator().manual_seed(seed)
    R = torch.randn([*shape, dim, dim], generator=gen, dtype=torch.float64)
    H = R @ R.transpose(-1, -2) + 0.1 * torch.eye(dim, dtype=torch.float64)
    comps = [H[..., i, i] for i in range(dim)] + [H[..., i, j] for i in range(dim) for j in range(i + 1, dim)]
    return torch.stack(comps, -1)[None], torch.block_diag(*H.reshape(-1, dim, dim))


@pytest.mark.parametrize("shape,bound", [((5,), "sliding"), ((4, 5), "sliding"), ((4, 5), ["dft", "zero"]), ((3, 3, 3), ["sliding", "zero", "dft"]),
                                         ((2, 1, 1), "sliding")], ids=str)
def test_solve_reaches_the_dense_solution(shape, bound):
    """CG run to a relative residual of 1e-13: the error is below cond(H + L) 1e-13 |x|, and with absolute = 0.3 and these
    weights cond < 1e4: the bar is 1e-9"""
    dim = len(shape)
    g = field(shape, 70 + dim)
    h, Hm = full_hessian(shape, 71)
    L = dense(entries(shape, bound, VOXELS[dim], **FIVE))
    assert float(torch.linalg.cond(Hm + L)) < 1e4
    for hess, M in ((None, L), (h, Hm + L)):
        want = torch.from_numpy(numpy.linalg.solve(M.numpy(), g.reshape(2, -1).T.numpy())).T.reshape(g.shape)
        x, info = interpol.regulariser_solve(g, hess, voxel_size=VOXELS[dim], bound=bound, max_iter=200, tolerance=1e-13,
                                             return_info=True, **FIVE)
        assert bool((info.residual <= 1e-13).all()) and bool((info.iterations > 0).all())
        assert_close(x, want, 1e-9, (shape, bound, hess is not None))


def test_preconditioner_is_the_interior_diagonal():
    for shape in [(7,), (5, 6), (5, 5, 5)]:
        dim = len(shape)
        for w in WEIGHTS:
            L = dense(entries(shape, "dft", VOXELS[dim], **w))
            o = 0
            for n in shape:
                o = o * n + 2
            want = [float(L[o * dim + c, o * dim + c]) for c in range(dim)]
            five = tuple(w.get(k, 0.) for k in ("absolute", "membrane", "bending", "shears", "div"))
            got = torch_kernels.regulariser_solve_centre(five, VOXELS[dim])
            assert numpy.allclose(got, want, rtol=1e-13, atol=0), (shape, w, got, want)
    # three weights still serve
    assert torch_kernels.regulariser_solve_centre((0.3, 0.7, 1.3), VOXELS[3]) == torch_kernels.regulariser_solve_centre((0.3, 0.7, 1.3, 0., 0.), VOXELS[3])


def test_solve_refuses_a_non_symmetric_L():
    g = field((4, 5), 72)
    for bound in ("dct2", "dst2", ["sliding", "dct2"], "replicate"):
        with pytest.raises(ValueError, match="symmetric"):
            interpol.regulariser_solve(g, bound=bound, shears=1.0)
        with pytest.raises(ValueError, match="symmetric"):
            interpol.regulariser_solve(g, bound=bound, membrane=1.0, div=1.0)
    # without elastic terms dct2 / dst2 serve as before, and sliding is new
    for bound in ("dct2", "dst2", "sliding", ["sliding", "dct2"]):
        interpol.regulariser_solve(g, bound=bound, membrane=1.0, max_iter=2)
    with pytest.raises(ValueError, match="positive"):
        interpol.regulariser_solve(g, bound="dft")


# ---------------------------------------------------------------------------------------------------------------------
# 3b. the fixed-count comparison of the device module: its cases, the host runs, and the runs that are not reproducible
# ---------------------------------------------------------------------------------------------------------------------
SOLVE_TOL = {torch.float32: 1e-5, torch.float64: 1e-11}
DEVICE_SHAPES = [(130,), (19, 11), (9, 5, 67), (3, 3, 3), (1, 2, 3), (2, 1, 1), (4, 2, 5), (6, 1, 7)]


def solve_close(got, want, tol):
    """error / bar of |got - want| <= tol |want| + tol max|want|, the worst element"""
    got = got.detach().cpu().double()
    assert got.shape == want.shape and bool(torch.isfinite(got).all())
    return float(((got - want).abs() / (tol * want.abs() + tol * float(want.abs().max()))).max())


def solve_cases(dim):
    """(weights, bound, voxel size, Hessian kind), by the logic of `cases_for` of tests/test_regulariser_solve_cpu.py: no singular
    system and cond(A) bounded a priori -- `absolute` = a bounds it by (a + ||L||) / a with ||L|| <= 4 (membrane + 2 shears + div)
    sum_e 1 / h_e^2 + 16 bending (sum_e 1 / h_e^2)^2 + (shears + div) (D - 1), at most 80 for the unit-voxel weights below: 800
    with a = 0.1; or the Hessian bounds it (eigenvalues of order 0.1)."""
    return [(dict(absolute=0.1, shears=0.6, div=0.9), "dft", 1., "none"), (dict(shears=0.6, div=0.9), "sliding", 1., "full"),
            (dict(absolute=0.1, membrane=0.7, shears=0.6, div=0.9), ["sliding", "zero", "dft"][:dim], 1., "diag"),
            (dict(absolute=0.1, bending=0.3, shears=0.6, div=0.9), "sliding", 1., "none"),
            (FIVE, "sliding", VOXELS[dim], "full"), (dict(absolute=0.3, membrane=0.7, bending=1.3), "sliding", 1., "diag"), (FIVE, "zero", 1., "none")]


_HOST = {}


def host_runs(key, g, h, kw, counts):
    """The composed algorithm on the host, computed once per case and shared: {(dtype, k): (x, iterations, residual)}, and
    {("moved", dtype, k): error / bar} -- how far the reference's OWN run in `dtype`, on a right-hand side moved by one unit
    roundoff of `dtype` (g (1 + u randn)), ends from its float64 run on g"""
    if key not in _HOST:
        runs = {}
        gen = torch.Generator().manual_seed(1)
        noise = torch.randn(g.shape, generator=gen, dtype=torch.float64)
        for dtype, u in ((torch.float64, 2.0 ** -52), (torch.float32, 2.0 ** -23)):
            for k in counts:
                hh = None if h is None else h.to(dtype)
                x, info = interpol.regulariser_solve(g.to(dtype), hh, max_iter=k, tolerance=0., return_info=True, **kw)
                runs[dtype, k] = (x.double(), info.iterations, info.residual)
                moved = interpol.regulariser_solve((g.double() * (1 + u * noise)).to(dtype), hh, max_iter=k, tolerance=0., **kw)
                runs["moved", dtype, k] = solve_close(moved, runs[torch.float64, k][0], SOLVE_TOL[dtype])
        _HOST[key] = runs
    return _HOST[key]


# (shape, index into solve_cases, dtype, iterations): the runs of conjugate gradients that are not reproducible in that
# precision whoever makes them -- tiny shapes (18 to 126 unknowns), where after 8 or 24 iterations the clusters of the spectrum
# are resolved and the next search direction is made of rounding errors (the FLOAT32_UNSTABLE_AT_24 / FLOAT64_UNSTABLE_AT_24 of
# tests/test_regulariser_solve_cpu.py, for these cases).  The reference's own run in that precision on a right-hand side moved by
# one unit roundoff ends 1.2 to 153 bars from its float64 run there, and at most 0.18 bars from it on every other (shape, case,
# dtype, count): test_unstable_runs_are_the_references_own asserts both.  The device module compares everything else.
UNSTABLE = {((3, 3, 3), 4, torch.float32, 24), ((1, 2, 3), 5, torch.float32, 8), ((4, 2, 5), 3, torch.float32, 24),
            ((4, 2, 5), 4, torch.float32, 24), ((4, 2, 5), 5, torch.float64, 24), ((4, 2, 5), 5, torch.float32, 24),
            ((6, 1, 7), 3, torch.float32, 24), ((6, 1, 7), 5, torch.float32, 24)}


def device_system(case, n):
    """the right-hand side, the Hessian argument and the keywords of case n on DEVICE_SHAPES[case] (float32 values: both
    precisions see the same system)"""
    import test_regulariser_solve_cpu as st
    shape = DEVICE_SHAPES[case]
    w, bound, vx, kind = solve_cases(len(shape))[n]
    g = field(shape, 100 * case + n, torch.float32)
    h = st.hessian_arg(shape, 100 * case + n + 1000, kind, torch.float32)[0]
    return g, h, dict(voxel_size=vx, bound=bound, **w)


@pytest.mark.parametrize("case", range(len(DEVICE_SHAPES)), ids=ids(DEVICE_SHAPES))
def test_unstable_runs_are_the_references_own(case):
    shape = DEVICE_SHAPES[case]
    assert all(sh in DEVICE_SHAPES and n < len(solve_cases(len(sh))) and k in (8, 24) for sh, n, _, k in UNSTABLE)
    for n in range(len(solve_cases(len(shape)))):
        g, h, kw = device_system(case, n)
        runs = host_runs((shape, n), g, h, kw, (1, 8, 24))
        for dtype in (torch.float64, torch.float32):
            for k in (1, 8, 24):
                off = max(runs["moved", dtype, k], solve_close(runs[dtype, k][0], runs[torch.float64, k][0], SOLVE_TOL[dtype]))
                if (shape, n, dtype, k) in UNSTABLE:
                    assert off > 1.0, (shape, n, dtype, k, off)
                else:
                    assert off <= 0.5, (shape, n, dtype, k, off)


# ---------------------------------------------------------------------------------------------------------------------
# 4. arguments
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    v = field((4, 5), 73)
    for fn in (interpol.regulariser, interpol.regulariser_energy, interpol.regulariser_solve):
        for name in ("shears", "div"):
            with pytest.raises(TypeError, match=name):
                fn(v, **{name: torch.tensor(1.0)})
            for bad in (-1.0, float("inf"), float("nan")):
                with pytest.raises(ValueError, match=name):
                    fn(v, **{name: bad})
        with pytest.raises(ValueError):
            fn(v, shears=1.0, bound="slide")
    with pytest.raises(ValueError):
        torch_kernels.regulariser_composed(v, (1.0, 1.0), [1., 1.], [6, 6])


def test_positional_calls_keep_their_meaning():
    v = field((4, 5), 74)
    assert torch.equal(interpol.regulariser(v, 0.3, 0.7, 1.3, [0.5, 1.25], "dct2"),
                       interpol.regulariser(v, absolute=0.3, membrane=0.7, bending=1.3, voxel_size=[0.5, 1.25], bound="dct2"))
    a = interpol.regulariser_solve(v, None, 0.3, 0.7, 0., 1., "dft", 3, 0., False)
    assert torch.equal(a, interpol.regulariser_solve(v, absolute=0.3, membrane=0.7, max_iter=3))


@pytest.mark.parametrize("bound", NAMES)
def test_zero_elastic_weights_change_nothing(bound):
    v = field((4, 5), 75)
    kw = dict(absolute=0.3, membrane=0.7, bending=1.3, voxel_size=[0.5, 1.25], bound=bound)
    assert torch.equal(interpol.regulariser(v, **kw), interpol.regulariser(v, shears=0., div=0., **kw))
    assert torch.equal(interpol.regulariser_energy(v, **kw), interpol.regulariser_energy(v, shears=0., div=0., **kw))
    if bound in ("zero", "dct2", "dst2", "dft"):
        assert torch.equal(interpol.regulariser_solve(v, max_iter=4, **kw), interpol.regulariser_solve(v, max_iter=4, shears=0., div=0., **kw))
    assert torch.equal(interpol.regulariser(v, shears=0., div=0.), torch.zeros_like(v))


def test_sliding_is_known_to_the_regulariser_only():
    vol = torch.zeros(1, 1, 4, 5)
    grid = torch.zeros(1, 4, 5, 2)
    with pytest.raises(ValueError, match="Unknown boundary condition sliding"):
        interpol.grid_pull(vol, grid, bound="sliding")
    with pytest.raises(ValueError, match="Unknown boundary condition sliding"):
        interpol.codes.bound_to_code("sliding")
    with pytest.raises(ValueError):
        interpol.jacobian(grid, bound="sliding")
    # absolute alone has no tap off the centre: sliding changes nothing
    v = field((4, 5), 76)
    assert torch.equal(interpol.regulariser(v, absolute=2.0, bound="sliding"), interpol.regulariser(v, absolute=2.0, bound="dct2"))


def test_bf16_fields_compute_in_float32_and_round_once():
    v = field((5, 4), 77).to(torch.bfloat16)
    E = entries((5, 4), "sliding", VOXELS[2], **FIVE)
    got = interpol.regulariser(v, voxel_size=VOXELS[2], bound="sliding", **FIVE)
    assert got.dtype == torch.bfloat16
    assert_close(got.float(), apply_entries(E, v.float()), 1e-2, "bf16")
