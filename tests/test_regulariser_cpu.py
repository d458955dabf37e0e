"""`interpol.regulariser` / `interpol.regulariser_energy`: the definition, the composed form and the host layers (no GPU).

Truth everywhere -- here and in tests/test_regulariser_gpu.py, which imports this module for it -- is the dense float64 matrix of

    (L v)_d = h_d^2 [ absolute v_d + membrane sum_e A_e v_d + bending ( sum_e B_e v_d + sum_{e != f} A_e A_f v_d ) ]

built in `spatial_matrix`: the 1-D matrices A_e = (-1, 2, -1) / h_e^2 and B_e = (1, -4, 6, -4, 1) / h_e^4 row by row from
`oracle.bound_index` / `oracle.bound_sign` (every tap through the tables, the centre included), assembled with Kronecker
products.  L is the same for every component up to h_d^2, so the (N x N) spatial matrix S is kept and L = S (x) diag(h^2).
Never the code under test.

Bar of the float64 comparisons: |got - want| <= 1e-11 |want| + 1e-11 max|want|.
"""
import pytest
import torch

import interpol
from interpol import autograd as iautograd
from oracle import oracle

BOUNDS = ["zero", "replicate", "dct1", "dct2", "dst1", "dst2", "dft"]
SYMMETRIC = ["zero", "dct2", "dst2", "dft"]
TAPS_A = {0: 2.0, -1: -1.0, 1: -1.0}
TAPS_B = {0: 6.0, -1: -4.0, 1: -4.0, -2: 1.0, 2: 1.0}
_CACHE = {}


def stencil_matrix(n, bound, taps):
    """(n x n) float64: row o holds sum_t taps[t] f~[o + t], f~[i] = sign(i) f[index(i)] by the oracle's tables"""
    code = BOUNDS.index(bound)
    M = torch.zeros(n, n, dtype=torch.float64)
    for o in range(n):
        for t, c in taps.items():
            s = oracle.bound_sign(code, o + t, n)
            M[o, oracle.bound_index(code, o + t, n)] += c * (1 if s is None else s)
    return M


def _kron_entries(mats, shape):
    """The non-zero entries (row, column, value) of the Kronecker product of one matrix per dimension (None: the identity),
    row-major"""
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


def spatial_matrix(shape, bound, absolute=0., membrane=0., bending=0., voxel_size=1.):
    """S (N x N, dense float64) with (L v)_d = h_d^2 S v_d; bound: a name or one per dim; voxel_size: a number or one per dim.
    S = absolute I + sum_e K_e(membrane A_e + bending B_e) + bending sum_{e != f} K_ef(A_e, A_f), K: the Kronecker product with
    identities along the other dimensions.  (The products are accumulated entry by entry: 3015^2 dense products would take
    a second each.)"""
    dim = len(shape)
    bound = [bound] * dim if isinstance(bound, str) else list(bound)
    vx = [float(voxel_size)] * dim if not isinstance(voxel_size, (list, tuple)) else [float(h) for h in voxel_size]
    key = (tuple(shape), tuple(bound), absolute, membrane, bending, tuple(vx))
    if key in _CACHE:
        return _CACHE[key]
    A = [stencil_matrix(n, b, TAPS_A) / h ** 2 for n, b, h in zip(shape, bound, vx)]
    B = [stencil_matrix(n, b, TAPS_B) / h ** 4 for n, b, h in zip(shape, bound, vx)]
    N = 1
    for n in shape:
        N *= n
    terms = [(torch.arange(N), torch.arange(N), torch.full([N], float(absolute), dtype=torch.float64))]
    for e in range(dim):
        one = [None] * dim
        one[e] = membrane * A[e] + bending * B[e]
        terms.append(_kron_entries(one, shape))
        for f in range(dim):
            if f != e and bending:
                two = [None] * dim
                two[e], two[f] = bending * A[e], A[f]
                terms.append(_kron_entries(two, shape))
    row, col, val = (torch.cat(x) for x in zip(*terms))
    S = torch.zeros(N * N, dtype=torch.float64).index_add_(0, row * N + col, val).reshape(N, N)
    while len(_CACHE) >= 8:                                              # (72 MB each at 9 x 5 x 67)
        _CACHE.pop(next(iter(_CACHE)))
    _CACHE[key] = S
    return S


def h2(dim, voxel_size=1.):
    vx = [float(voxel_size)] * dim if not isinstance(voxel_size, (list, tuple)) else [float(h) for h in voxel_size]
    return torch.tensor(vx, dtype=torch.float64) ** 2


def apply_dense(S, v, voxel_size=1., transpose=False):
    """L v (or L^T v) in float64: v (B, *shape, D) -> the same shape"""
    dim = v.shape[-1]
    flat = v.double().reshape(v.shape[0], -1, dim)
    M = S.T if transpose else S
    return (torch.einsum("on,bnd->bod", M, flat) * h2(dim, voxel_size)).reshape(v.shape)


def energy_dense(S, v, voxel_size=1.):
    return 0.5 * (v.double() * apply_dense(S, v, voxel_size)).reshape(v.shape[0], -1).sum(1)


def taps_abs_sum(dim, absolute=0., membrane=0., bending=0., voxel_size=1.):
    """sum of the absolute coefficients of the taps of one row of L, before taps that fold onto one point are merged (an upper bound of
    ||L||_inf): the size of the terms that cancel where they do"""
    hh = h2(dim, voxel_size)
    a = 1 / hh
    mixed = float(a.sum() ** 2 - (a * a).sum())
    return float(hh.max()) * (absolute + membrane * 4 * float(a.sum()) + bending * 16 * (float((a * a).sum()) + mixed))


def norm_inf(S, dim, voxel_size=1.):
    """||L||_inf of the full matrix S (x) diag(h^2)"""
    return float(S.abs().sum(1).max()) * float(h2(dim, voxel_size).max())


def field(shape, seed, dtype=torch.float64, B=2):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn([B, *shape, len(shape)], generator=gen, dtype=torch.float64).to(dtype)


def assert_close(got, want, tol, what, cancelled=None):
    """`cancelled`: taps_abs_sum max|v|, the size of the terms that cancel -- the bar where the truth is identically zero (every
    extent is 1 under a bound that repeats the one value: all stencils cancel and no relative bar applies to the rounding left)"""
    got = got.detach().cpu().double()
    err = (got - want).abs()
    allow = tol * want.abs() + tol * float(want.abs().max())
    if cancelled is not None and not bool(want.any()):
        allow = torch.full_like(want, tol * cancelled)
    assert got.shape == want.shape and bool(torch.isfinite(got).all()), what
    assert bool((err <= allow).all()), (what, float((err / allow.clamp_min(1e-300)).max()))


SHAPES = [(7,), (5, 4), (3, 4, 5), (1,), (2,), (1, 2, 3)]
VOXELS = {1: [1.5], 2: [0.5, 1.25], 3: [2.0, 0.75, 1.5]}
WEIGHTS = [dict(absolute=0.3, membrane=0.7, bending=1.3), dict(membrane=1.0), dict(bending=1.0), dict(absolute=2.0)]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the composed form is the dense matrix
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_composed_form_matches_the_dense_matrix(shape):
    dim = len(shape)
    v = field(shape, 10 + dim)
    mixed = ["dct2", "dst1", "zero"][:dim]
    for bound in BOUNDS + [mixed]:
        for w in WEIGHTS:
            for vx in (1., VOXELS[dim]):
                S = spatial_matrix(shape, bound, voxel_size=vx, **w)
                what = (shape, bound, w, vx)
                got = interpol.regulariser(v, voxel_size=vx, bound=bound, **w)
                assert got.dtype == v.dtype
                assert_close(got, apply_dense(S, v, vx), 1e-11, what, cancelled=taps_abs_sum(dim, voxel_size=vx, **w) * float(v.abs().max()))
                E = interpol.regulariser_energy(v, voxel_size=vx, bound=bound, **w)
                assert E.shape == (2,)
                want = energy_dense(S, v, vx)
                # relative to the sum of the absolute terms of the quadratic form (the energy itself may cancel to nothing)
                scale = 0.5 * taps_abs_sum(dim, voxel_size=vx, **w) * float(v.abs().max()) * v.abs().reshape(2, -1).sum(1)
                assert bool(((E.double() - want).abs() <= 1e-11 * scale).all()), what


def test_stencil_coefficients_in_3d():
    """unit voxels, bending = 1: 25 points, the centre is 42 and the absolute coefficients sum to 144"""
    S = spatial_matrix((7, 7, 7), "dft", bending=1.)
    row = S[(3 * 7 + 3) * 7 + 3]
    assert int((row != 0).sum()) == 25 and float(row.max()) == 42. and float(row.abs().sum()) == 144. and float(row.sum()) == 0.


# ---------------------------------------------------------------------------------------------------------------------
# 2. L itself
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(7,), (5, 4), (3, 4, 5), (2,), (1, 2, 3)], ids=str)
def test_L_is_symmetric_psd_for_the_four_symmetric_bounds(shape):
    """what the fused backward (L^T = L) rests on"""
    dim = len(shape)
    for bound in SYMMETRIC + [["dct2", "dft", "zero"][:dim], ["dst2", "zero", "dft"][:dim]]:
        for w in WEIGHTS:
            S = spatial_matrix(shape, bound, voxel_size=VOXELS[dim], **w)
            assert torch.equal(S, S.T), (shape, bound, w)
            assert float(torch.linalg.eigvalsh(S).min()) >= -1e-12 * float(S.abs().max()), (shape, bound, w)


def test_L_is_not_symmetric_for_the_other_three():
    for bound, n in (("replicate", 3), ("dct1", 3), ("dst1", 2)):
        S = spatial_matrix((n,), bound, membrane=1., bending=1.)
        assert not torch.equal(S, S.T), bound
    # (the membrane term alone is symmetric under replicate -- the Neumann Laplacian -- its bending term is what breaks it)
    S = spatial_matrix((5,), "replicate", membrane=1.)
    assert torch.equal(S, S.T)


def test_bending_is_the_stencil_on_the_extended_field_not_A_twice():
    for bound in ("zero", "replicate"):
        for n in range(2, 9):
            A, B = stencil_matrix(n, bound, TAPS_A), stencil_matrix(n, bound, TAPS_B)
            assert not torch.equal(A @ A, B), (bound, n)
    # ... while under the periodic bound the two agree
    assert torch.equal(stencil_matrix(8, "dft", TAPS_A) @ stencil_matrix(8, "dft", TAPS_A), stencil_matrix(8, "dft", TAPS_B))


# ---------------------------------------------------------------------------------------------------------------------
# 3. autograd on the CPU route
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bound", ["dct2", "replicate", "dst1"])
def test_gradcheck_and_gradgradcheck(bound):
    kw = dict(absolute=0.3, membrane=0.7, bending=1.3, voxel_size=[0.5, 1.25], bound=bound)
    v = field((3, 4), 3, B=1).requires_grad_()
    assert (bound in SYMMETRIC) == iautograd._regulariser_symmetric([BOUNDS.index(bound)] * 2)
    for fn in (interpol.regulariser, interpol.regulariser_energy):
        assert torch.autograd.gradcheck(lambda x: fn(x, **kw), (v,))
        assert torch.autograd.gradgradcheck(lambda x: fn(x, **kw), (v,))


@pytest.mark.parametrize("bound", BOUNDS)
def test_gradients_are_the_transposed_matrix(bound):
    shape, vx = (3, 4, 5), VOXELS[3]
    w = dict(absolute=0.3, membrane=0.7, bending=1.3)
    S = spatial_matrix(shape, bound, voxel_size=vx, **w)
    v = field(shape, 5).requires_grad_()
    g = field(shape, 6)
    ge = torch.tensor([0.7, -1.9], dtype=torch.float64)
    got, = torch.autograd.grad(interpol.regulariser(v, voxel_size=vx, bound=bound, **w), v, g)
    assert_close(got, apply_dense(S, g, vx, transpose=True), 1e-11, bound)
    got, = torch.autograd.grad(interpol.regulariser_energy(v, voxel_size=vx, bound=bound, **w), v, ge)
    want = 0.5 * (apply_dense(S, v.detach(), vx) + apply_dense(S, v.detach(), vx, transpose=True)) * ge.reshape(2, 1, 1, 1, 1)
    assert_close(got, want, 1e-11, bound)


# ---------------------------------------------------------------------------------------------------------------------
# 4. shape conventions and argument checks
# ---------------------------------------------------------------------------------------------------------------------
def test_batch_dimensions_are_free():
    kw = dict(membrane=1., bending=0.5, bound="dct2")
    v = field((4, 5), 7, B=6).reshape(2, 3, 4, 5, 2)
    out = interpol.regulariser(v, **kw)
    E = interpol.regulariser_energy(v, **kw)
    assert out.shape == v.shape and E.shape == (2, 3)
    one = interpol.regulariser(v[1, 2], **kw)                           # no batch at all
    assert one.shape == (4, 5, 2) and torch.equal(one, out[1, 2])
    e1 = interpol.regulariser_energy(v[1, 2], **kw)
    assert e1.shape == () and torch.equal(e1, E[1, 2])
    # D = 4 and 16-bit fields: the composed form (float32 inside, rounded once)
    v4 = torch.randn(2, 3, 3, 2, 3, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    S = spatial_matrix((3, 3, 2, 3), "dft", membrane=1., bending=0.5)
    assert_close(interpol.regulariser(v4, membrane=1., bending=0.5), apply_dense(S, v4), 1e-11, "4-D")
    vb = field((4, 5), 8).bfloat16()
    out = interpol.regulariser(vb, **kw)
    assert out.dtype == torch.bfloat16 and interpol.regulariser_energy(vb, **kw).dtype == torch.bfloat16
    assert_close(out.float(), apply_dense(spatial_matrix((4, 5), "dct2", membrane=1., bending=0.5), vb.float()), 1e-2, "bf16")


def test_argument_errors():
    v = field((4, 5), 9)
    for name in ("absolute", "membrane", "bending"):
        with pytest.raises(ValueError):
            interpol.regulariser(v, **{name: -1.})
        with pytest.raises(ValueError):
            interpol.regulariser_energy(v, **{name: -1.})
        with pytest.raises(TypeError):
            interpol.regulariser(v, **{name: torch.tensor(1.)})
    with pytest.raises(ValueError):
        interpol.regulariser(torch.zeros(2, 4, 5, 3, dtype=torch.float64)[0], membrane=1.)       # (4, 5, 3): no 3-D field
    with pytest.raises(ValueError):
        interpol.regulariser(torch.zeros(2, 4, 5, 2, dtype=torch.int64), membrane=1.)
    with pytest.raises(ValueError):
        interpol.regulariser_energy(torch.zeros(2, 4, 5, 2, dtype=torch.int32), membrane=1.)
    for vx in (0., -1., [1., 2., 3.], [1., 0.]):
        with pytest.raises(ValueError):
            interpol.regulariser(v, membrane=1., voxel_size=vx)


def test_all_weights_zero():
    v = field((4, 5), 11, B=6).reshape(2, 3, 4, 5, 2)
    out = interpol.regulariser(v)
    assert out.shape == v.shape and out.dtype == v.dtype and not bool(out.any())
    E = interpol.regulariser_energy(v)
    assert E.shape == (2, 3) and E.dtype == v.dtype and not bool(E.any())
