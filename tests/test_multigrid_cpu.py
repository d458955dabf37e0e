"""`interpol.regulariser_solve(preconditioner='multigrid')`: the V-cycle, the composed form and the host layers (no GPU).

Truth -- here and in tests/test_multigrid_gpu.py, which imports this module for it -- is a float64 restatement of the algorithm
with explicit matrices, written without interpol/ops.py or interpol/torch_kernels.py:

  L_l   the level operator, column by column: `interpol.regulariser` applied to the identity fields of the level's lattice with
        the weights times kappa_l and the voxel sizes h_l (every coupling between components included);
  A_l = L_l + blockdiag(H_l),  M_l = H_l + diag(c(kappa_l weights, h_l)) inverted block by block with torch.linalg.inv;
  P_l   an explicit matrix: per component the Kronecker product of one 1-D matrix per dimension (`prolong_1d`, the identity
        for a dimension that is not halved), times s_c;  restriction is P_l^T -- the matrix, not a second rule;
  H_{l+1} = S (sum of the children) S on the (N, D, D) blocks.

`vcycle` applies V to the columns of a matrix, so V itself is `vcycle` of the identity.  `pcg` is the documented conjugate-gradient
loop for ONE item with any preconditioner (the Jacobi one gives the iteration counts of the comparison).

The fixed inputs are those of tests/test_regulariser_solve_cpu.py: g = field(shape, seed), B = 2, item 0 with the full Hessian
0.5 R R^T / D and item 1 with the diagonal 0.2 rand (`hessian_arg`); 'broadcast' hands over item 0's full Hessian without a batch
dimension, which then serves both items.  No singular system: bending or membrane alone under dft / dct2 comes with a Hessian
or with `absolute`.

Bars: float64 |got - want| <= 1e-11 |want| + 1e-11 max|want| (the project's).
"""
import math

import pytest
import torch

import interpol
import test_regulariser_cpu as truth
import test_regulariser_solve_cpu as st

TOL64 = 1e-11
OMEGA = 0.5
COARSEST_SWEEPS = 8
WEIGHT_NAMES = ("absolute", "membrane", "bending", "shears", "div")
_CACHE = {}


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
def halved_dims(shape):
    return [n % 2 == 0 and n // 2 >= 4 for n in shape]


def level_shapes(shape):
    """[(shape, halved)] from level 0 to the last level (halved: all False there)"""
    out, shape = [], list(shape)
    while True:
        hv = halved_dims(shape)
        out.append((tuple(shape), hv))
        if not any(hv):
            return out
        shape = [n // 2 if y else n for n, y in zip(shape, hv)]


def centre5(w, vx):
    """c_d of the docstring of `interpol.regulariser_solve`, with all five weights"""
    a, m, b, sh, dv = (float(w.get(k, 0.)) for k in WEIGHT_NAMES)
    D = len(vx)
    inv2 = [1.0 / (h * h) for h in vx]
    common = a + (m + sh) * sum(2 * x for x in inv2) + b * (sum(6 * x * x for x in inv2)
                                                           + sum(4 * inv2[e] * inv2[f] for e in range(D) for f in range(D) if e != f))
    return torch.tensor([vx[d] ** 2 * (common + (sh + dv) * 2 * inv2[d]) for d in range(D)], dtype=torch.float64)


def dense_L(shape, w, vx, bound, sparse=False):
    """L (N D x N D) of one level from `interpol.regulariser` on identity fields, unknowns ordered point by point; sparse: CSR,
    assembled in slabs of columns so that no dense N D x N D array exists"""
    D = len(shape)
    n = math.prod(shape) * D
    slab = 1024 if sparse else n
    parts = []
    for i0 in range(0, n, slab):
        m = min(slab, n - i0)
        eye = torch.zeros(m, n, dtype=torch.float64)
        eye[torch.arange(m), i0 + torch.arange(m)] = 1.0
        cols = interpol.regulariser(eye.reshape(m, *shape, D), voxel_size=list(vx), bound=bound, **w).reshape(m, n)   # rows of L^T
        parts.append(cols.to_sparse() if sparse else cols)
    LT = torch.cat(parts)
    return LT.t().to_sparse_csr() if sparse else LT.t().contiguous()


def prolong_1d(nf, bound):
    """(nf x nf/2): fine i = 3/4 e[i >> 1] + 1/4 e[(i >> 1) -+ 1], a coarse index out of range extended by `bound`"""
    nc = nf // 2
    P = torch.zeros(nf, nc, dtype=torch.float64)
    for i in range(nf):
        j = i >> 1
        k = j - 1 if i % 2 == 0 else j + 1
        P[i, j] += 0.75
        s = 1.0
        if k < 0 or k >= nc:
            if bound == "dft":
                k %= nc
            elif bound == "dct2":
                k = j                                                # (reflection about the edge: -1 -> 0, nc -> nc - 1)
            elif bound == "dst2":
                k, s = j, -1.0
            elif bound == "zero":
                k, s = j, 0.0
            else:
                raise ValueError(bound)
        P[i, k] += 0.25 * s
    return P


def restrict_1d_gather(nf, bound):
    """(nf/2 x nf): the gather rule of the issue -- coarse j sums fine 2j - 1, 2j, 2j + 1, 2j + 2 with 1/4, 3/4, 3/4, 1/4, a fine
    index out of range extended by `bound` on the FINE field"""
    nc = nf // 2
    R = torch.zeros(nc, nf, dtype=torch.float64)
    for j in range(nc):
        for t, q in zip(range(2 * j - 1, 2 * j + 3), (0.25, 0.75, 0.75, 0.25)):
            i, s = t, 1.0
            if t < 0 or t >= nf:
                if bound == "dft":
                    i = t % nf
                elif bound in ("dct2", "dst2"):
                    i = -1 - t if t < 0 else 2 * nf - 1 - t
                    s = -1.0 if bound == "dst2" else 1.0
                elif bound == "zero":
                    i, s = 0, 0.0
            R[j, i] += q * s
    return R


def bound_of(bound, d, c):
    """the extension of component c along dimension d"""
    b = bound if isinstance(bound, str) else bound[d]
    if b == "sliding":
        return "dst2" if c == d else "dct2"
    return b


def kron_all(mats):
    out = mats[0]
    for m in mats[1:]:
        out = torch.kron(out, m)
    return out


def dense_P(shape, hv, bound, one=prolong_1d, transpose=False):
    """P (N_f D x N_c D), or with one=restrict_1d_gather and transpose=True the gather restriction (N_c D x N_f D)"""
    D = len(shape)
    nf = math.prod(shape)
    nc = math.prod(n // 2 if y else n for n, y in zip(shape, hv))
    out = torch.zeros((nc if transpose else nf) * D, (nf if transpose else nc) * D, dtype=torch.float64)
    for c in range(D):
        mats = [one(shape[d], bound_of(bound, d, c)) if hv[d] else torch.eye(shape[d], dtype=torch.float64) for d in range(D)]
        out[c::D, c::D] = kron_all(mats) * (2.0 if hv[c] else 1.0)
    return out


def coarsen_blocks(Hd, shape, hv):
    """(N_f, D, D) -> (N_c, D, D): S (sum of the children) S"""
    D = len(shape)
    H = Hd.reshape(*shape, D, D)
    for d, y in enumerate(hv):
        if y:
            s = list(H.shape)
            H = H.reshape(s[:d] + [s[d] // 2, 2] + s[d + 1:]).sum(d + 1)
    S = torch.tensor([2.0 if y else 1.0 for y in hv], dtype=torch.float64)
    return (H * S[:, None] * S[None, :]).reshape(-1, D, D)


def add_blocks(L, Hd, sparse=False):
    N, D = Hd.shape[:2]
    if sparse:
        o = torch.arange(N)
        rows = (o[:, None, None] * D + torch.arange(D)[None, :, None]).expand(N, D, D).reshape(-1)
        cols = (o[:, None, None] * D + torch.arange(D)[None, None, :]).expand(N, D, D).reshape(-1)
        Hs = torch.sparse_coo_tensor(torch.stack([rows, cols]), Hd.reshape(-1), (N * D, N * D)).coalesce()
        return (L.to_sparse_coo() + Hs).coalesce().to_sparse_csr()
    A = L.clone().reshape(N, D, N, D)
    n = torch.arange(N)
    A[n, :, n, :] += Hd
    return A.reshape(N * D, N * D)


def build_levels(shape, bound, w, vx, Hd, sparse=False):
    """the levels of the cycle for ONE item: Hd (N, D, D) float64 -> [dict(A, Minv (N,D,D), P | None)]"""
    D = len(shape)
    vx = st.voxels(D, vx)
    levels, kappa, Hd = [], 1.0, Hd.double()
    for shp, hv in level_shapes(shape):
        wk = {k: kappa * float(v) for k, v in w.items()}
        key = ("L", shp, tuple(sorted(wk.items())), tuple(vx), str(bound), sparse)
        if key not in _CACHE:
            _CACHE[key] = dense_L(shp, wk, vx, bound, sparse)
        lev = dict(A=add_blocks(_CACHE[key], Hd, sparse), Minv=torch.linalg.inv(Hd + torch.diag(centre5(wk, vx))), P=None)
        levels.append(lev)
        if not any(hv):
            return levels
        P = dense_P(shp, hv, bound)
        lev["P"] = P.to_sparse_csr() if sparse else P
        lev["PT"] = P.t().to_sparse_csr() if sparse else P.t().contiguous()
        Hd = coarsen_blocks(Hd, shp, hv)
        vx = [2 * h if y else h for h, y in zip(vx, hv)]
        kappa *= 2 ** sum(hv)


def vcycle(levels, r, nu=2, level=0):
    """V r for the columns of r (n x m)"""
    lev = levels[level]
    A, Minv = lev["A"], lev["Minv"]
    N, D = Minv.shape[:2]
    Mi = lambda v: torch.einsum("nde,nem->ndm", Minv, v.reshape(N, D, -1)).reshape(v.shape)
    last = lev["P"] is None
    x = OMEGA * Mi(r)
    for _ in range((COARSEST_SWEEPS if last else nu) - 1):
        x = x + OMEGA * Mi(r - A @ x)
    if last:
        return x
    d = r - A @ x
    x = x + lev["P"] @ vcycle(levels, lev["PT"] @ d, nu, level + 1)
    for _ in range(nu):
        x = x + OMEGA * Mi(r - A @ x)
    return x


def dense_V(levels, nu=2):
    n = levels[0]["Minv"].shape[0] * levels[0]["Minv"].shape[1]
    return vcycle(levels, torch.eye(n, dtype=torch.float64), nu)


def pcg(A, prec, g, max_iter, tolerance=0., keep=()):
    """the documented loop for ONE item: A (n x n), prec r -> z, g (n) -> x, iterations, residual, {k: x after min(k, its)}"""
    dot = lambda a, b: float((a * b).sum())
    x, r = torch.zeros_like(g), g.clone()
    z = prec(r)
    p = z.clone()
    rho, gamma = dot(r, z), dot(g, g)
    its, sigma, kept = 0, 0.0, {}
    for _ in range(max_iter if gamma != 0 else 0):
        q = (A @ p[:, None])[:, 0]
        pi = dot(p, q)
        if pi <= 0 or rho <= 0:
            break
        alpha = rho / pi
        x, r = x + alpha * p, r - alpha * q
        z = prec(r)
        rho1, sigma, its = dot(r, z), dot(r, r), its + 1
        if its in keep:
            kept[its] = x
        if sigma <= tolerance ** 2 * gamma:
            break
        p, rho = z + (rho1 / rho) * p, rho1
    return x, its, (math.sqrt(sigma / gamma) if its else 0.0), {k: kept.get(k, x) for k in keep}


def multigrid_prec(levels, nu=2):
    return lambda r: vcycle(levels, r[:, None], nu)[:, 0]


def jacobi_prec(levels):
    Minv = levels[0]["Minv"]
    return lambda r: torch.einsum("nde,ne->nd", Minv, r.reshape(Minv.shape[:2])).reshape(-1)


# ---------------------------------------------------------------------------------------------------------------------
# the cases (shared with the device tests)
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = [(16,), (16, 12), (7, 16), (5, 7), (16, 8, 10)]
IDS = ["x".join(map(str, s)) for s in SHAPES]
ELASTIC = dict(membrane=0.5, shears=1.0, div=2.0)
ITERATIONS = (1, 2, 4)


def cases_for(shape):
    """(weights, bound, voxel size, Hessian kind): every allowed bound, a per-dimension mix, the Hessian none / diagonal / full /
    broadcast, elastic weights under dft and sliding, anisotropic voxels -- (2.0, 0.75, 1.5) in 3-D"""
    dim = len(shape)
    mix = ["dct2", "zero", "dft"][:dim] if dim > 1 else "dst2"
    vx = [2.0, 0.75, 1.5][:dim]
    cases = [(dict(bending=1.0), "dft", 1., "full"),
             (dict(absolute=0.1, membrane=1.0), "dct2", 1., "none"),
             (dict(membrane=0.7, bending=0.3), "dst2", 1., "diag"),
             (st.ALL, "zero", vx, "broadcast"),
             (dict(absolute=0.2, bending=1.0), "sliding", vx, "none"),
             (dict(membrane=0.7, bending=1.3), mix, 1., "full")]
    if dim > 1:
        cases += [(ELASTIC, "dft", 1., "diag"), (dict(bending=0.5, **ELASTIC), "sliding", vx, "full"),
                  (dict(absolute=0.1, **ELASTIC), ["sliding", "dft", "zero"][:dim], 1., "none")]
    if dim == 3:
        # (3 840 unknowns: the dense levels of one case take seconds; dct2, dst2, the mixes and elastic under dft are held in 1-D / 2-D)
        cases = [cases[i] for i in (0, 3, 7)]
    return cases


def system(shape, seed, bound, w, vx, kind, dtype=torch.float64):
    """the arguments of one case in `dtype` and the (2, N, D, D) float64 Hessians they stand for, as the device sees them"""
    dim = len(shape)
    g = truth.field(shape, seed, dtype)
    h, Hd = st.hessian_arg(shape, seed + 1000, "full" if kind == "broadcast" else kind, dtype)
    if kind == "broadcast":
        h, Hd = h[0], torch.stack([Hd[0], Hd[0]])
    return dict(g=g, h=h, Hd=Hd.reshape(2, -1, dim, dim), kw=dict(voxel_size=vx, bound=bound, **w), shape=shape, bound=bound, w=w, vx=vx)


def levels_of(key, sy, sparse=False):
    """the two level lists of a case (one per item), built once"""
    if ("levels", key) not in _CACHE:
        _CACHE[("levels", key)] = [build_levels(sy["shape"], sy["bound"], sy["w"], sy["vx"], sy["Hd"][b], sparse) for b in range(2)]
    return _CACHE[("levels", key)]


def want_after(key, sy, keep=ITERATIONS, nu=2):
    """{k: (2, *shape, D)} after k iterations of the restated multigrid conjugate gradients, computed once per case"""
    if ("want", key, nu) not in _CACHE:
        g = sy["g"].double()
        per = []
        for b, levels in enumerate(levels_of(key, sy)):
            per.append(pcg(levels[0]["A"], multigrid_prec(levels, nu), g[b].reshape(-1), max(keep), keep=keep)[3])
        _CACHE[("want", key, nu)] = {k: torch.stack([per[b][k] for b in range(2)]).reshape(g.shape) for k in keep}
    return _CACHE[("want", key, nu)]


def prototype_system(dtype=torch.float64):
    """64 x 64, bending = 1, dft, and a seeded sparse positive semi-definite H: at three voxels in ten H = G G^T with G = 0.3
    randn(D, 2), elsewhere 0 (definite together with L, whose null space is the constants).  One item; -> (g (1,64,64,2), the
    packed full Hessian (1,64,64,3), Hd (N,2,2) float64)"""
    shape, D = (64, 64), 2
    gen = torch.Generator().manual_seed(0)
    G = 0.3 * torch.randn([*shape, D, 2], generator=gen, dtype=torch.float64)
    G = G * (torch.rand(shape, generator=gen, dtype=torch.float64) < 0.3)[..., None, None]
    h = st.pack(G @ G.transpose(-1, -2))[None].to(dtype)
    g = torch.randn([1, *shape, D], generator=gen, dtype=torch.float64).to(dtype)
    return g, h, st.unpack(h[0].double(), D).reshape(-1, D, D)


def prototype_counts(tolerance=1e-6):
    """(iterations of the restated multigrid CG, of the restated Jacobi CG capped at 400) to `tolerance` on `prototype_system`"""
    if ("proto", tolerance) not in _CACHE:
        g, _, Hd = prototype_system()
        levels = build_levels((64, 64), "dft", dict(bending=1.0), 1., Hd, sparse=True)
        A, b = levels[0]["A"], g.reshape(-1)
        mg = pcg(A, multigrid_prec(levels), b, 100, tolerance)[1]
        jac = pcg(A, jacobi_prec(levels), b, 400, tolerance)[1]
        _CACHE[("proto", tolerance)] = (mg, jac)
    return _CACHE[("proto", tolerance)]


# ---------------------------------------------------------------------------------------------------------------------
# 1. properties of the restatement
# ---------------------------------------------------------------------------------------------------------------------
def test_the_gather_restriction_is_the_transpose_of_the_prolongation():
    for bound in ("zero", "dft", "dct2", "dst2"):
        for nf in (8, 10, 16):
            assert torch.equal(restrict_1d_gather(nf, bound), prolong_1d(nf, bound).t()), (bound, nf)
    for shape, bound in (((8, 10), "sliding"), ((16, 12), ["sliding", "dft"]), ((8, 7, 12), ["dct2", "sliding", "sliding"]),
                         ((16, 8, 10), "sliding"), ((16, 12), ["zero", "dst2"])):
        hv = halved_dims(shape)
        P = dense_P(shape, hv, bound)
        R = dense_P(shape, hv, bound, one=restrict_1d_gather, transpose=True)
        assert torch.equal(R, P.t()), (shape, bound)
    # sliding really is per component: dst2 for c = d, dct2 otherwise
    P = dense_P((8, 8), [True, True], "sliding")
    assert float(P[0, 0]) == 2 * 0.5 * 1.0 and float(P[1, 1]) == 2 * 1.0 * 0.5


# (the whole matrix V takes N D columns through the cycle: in 3-D on (8, 8, 10), two levels, instead of (16, 8, 10))
@pytest.mark.parametrize("shape", SHAPES[:-1] + [(8, 8, 10)], ids=IDS[:-1] + ["8x8x10"])
def test_the_dense_cycle_is_symmetric_positive_definite(shape):
    for n, (w, bound, vx, kind) in enumerate(cases_for(shape)):
        sy = system(shape, 300 + n, bound, w, vx, kind)
        for levels in levels_of((shape, n), sy):
            V = dense_V(levels)
            assert float((V - V.t()).abs().max()) <= 1e-12 * float(V.abs().max()), (shape, n)
            assert float(torch.linalg.eigvalsh(0.5 * (V + V.t()))[0]) > 0, (shape, n)
    assert len(level_shapes((16, 12))) == 3 and level_shapes((16, 12))[1] == ((8, 6), [True, False])
    assert len(level_shapes((5, 7))) == 1


# ---------------------------------------------------------------------------------------------------------------------
# 2. the composed route against the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_fixed_iteration_counts_match_the_restated_algorithm(shape):
    worst = 0.0
    for n, (w, bound, vx, kind) in enumerate(cases_for(shape)):
        sy = system(shape, 300 + n, bound, w, vx, kind)
        want = want_after((shape, n), sy)
        for k in ITERATIONS:
            got, info = interpol.regulariser_solve(sy["g"], sy["h"], max_iter=k, preconditioner="multigrid", return_info=True, **sy["kw"])
            assert got.dtype == torch.float64 and got.shape == sy["g"].shape
            assert info.iterations.shape == (2,) and bool((info.iterations <= k).all())
            ratio = st.close(got, want[k], TOL64)
            worst = max(worst, ratio)
            assert ratio <= 1.0, (shape, w, bound, vx, kind, k, ratio)
    print("multigrid, fixed counts %s: worst error / bar = %.3g" % (shape, worst))


def test_smoothing_is_the_number_of_sweeps():
    shape = (16, 12)
    w, bound, vx, kind = cases_for(shape)[0]
    sy = system(shape, 300, bound, w, vx, kind)
    for nu in (1, 3):
        want = want_after((shape, 0), sy, (2,), nu)[2]
        got = interpol.regulariser_solve(sy["g"], sy["h"], max_iter=2, preconditioner="multigrid", smoothing=nu, **sy["kw"])
        assert st.close(got, want, TOL64) <= 1.0, nu


# ---------------------------------------------------------------------------------------------------------------------
# 3. what the preconditioner is for
# ---------------------------------------------------------------------------------------------------------------------
def test_multigrid_needs_a_quarter_of_the_iterations_of_jacobi():
    mg, jac = prototype_counts()
    print("64 x 64, bending, dft, to 1e-6: multigrid %d iterations, jacobi %d (capped at 400)" % (mg, jac))
    assert 4 * mg <= jac, (mg, jac)
    g, h, _ = prototype_system()
    x, info = interpol.regulariser_solve(g, h, bending=1.0, bound="dft", max_iter=100, tolerance=1e-6, preconditioner="multigrid",
                                         return_info=True)
    assert abs(int(info.iterations[0]) - mg) <= 1 and float(info.residual[0]) <= 1e-6, (info.iterations, mg)


# ---------------------------------------------------------------------------------------------------------------------
# 4. arguments
# ---------------------------------------------------------------------------------------------------------------------
def test_arguments():
    shape = (8, 6)
    g = truth.field(shape, 400)
    h, _ = st.hessian_arg(shape, 401, "full")
    ok = dict(membrane=1.0, bound="dct2", max_iter=3)
    for bad in ("ilu", "Multigrid", None, 1):
        with pytest.raises(ValueError):
            interpol.regulariser_solve(g, h, preconditioner=bad, **ok)
    for bad in (0, -1, 2.0, True, None, "2"):
        with pytest.raises(ValueError):
            interpol.regulariser_solve(g, h, preconditioner="multigrid", smoothing=bad, **ok)
        with pytest.raises(ValueError):
            interpol.regulariser_solve(g, h, smoothing=bad, **ok)
    with pytest.raises(ValueError):
        interpol.regulariser_solve(g, h, preconditioner="multigrid", **dict(ok, bound="dct1"))
    with pytest.raises(ValueError):
        interpol.regulariser_solve(g, h, preconditioner="multigrid", shears=1.0, **ok)          # elastic under dct2
    plain, info0 = interpol.regulariser_solve(g, h, return_info=True, **ok)
    named, info1 = interpol.regulariser_solve(g, h, return_info=True, preconditioner="jacobi", smoothing=5, **ok)
    assert torch.equal(plain, named) and torch.equal(info0.iterations, info1.iterations) and torch.equal(info0.residual, info1.residual)
    assert not hasattr(interpol, "regulariser_vcycle")
    assert interpol.backend.fused_regulariser_multigrid is True


def test_other_dtypes_dimensions_and_batches():
    shape = (16, 8)
    g = truth.field(shape, 410, torch.bfloat16)
    h, _ = st.hessian_arg(shape, 411, "full", torch.bfloat16)
    kw = dict(membrane=0.7, bending=0.3, bound=["zero", "dft"], max_iter=6, preconditioner="multigrid")
    x = interpol.regulariser_solve(g, h, **kw)
    ref = interpol.regulariser_solve(g.float(), h.float(), **kw)
    assert x.dtype == torch.bfloat16 and ref.dtype == torch.float32
    assert float((x.float() - ref).abs().max()) <= 1e-2 * float(ref.abs().max())
    # four dimensions: converged, against the dense solve
    shape = (8, 3, 2, 3)
    g = truth.field(shape, 420)
    h, Hd = st.hessian_arg(shape, 421, "full")
    w = dict(absolute=0.1, membrane=1.0)
    S = truth.spatial_matrix(shape, "dft", **w)
    got = interpol.regulariser_solve(g, h, bound="dft", max_iter=60, preconditioner="multigrid", **w)
    for b in range(2):
        A = st.dense_matrix(S, truth.h2(4), Hd[b].reshape(-1, 4, 4))
        want = torch.linalg.solve(A, g[b].reshape(-1)).reshape(g[b].shape)
        assert float((got[b] - want).abs().max()) <= TOL64 * float(want.abs().max())
    # leading batch dimensions fold; an item gives the same values alone
    shape = (8, 6)
    g = truth.field(shape, 430)
    h, _ = st.hessian_arg(shape, 431, "diag")
    kw = dict(bending=1.0, bound="dft", max_iter=3, preconditioner="multigrid")
    x = interpol.regulariser_solve(g, h, **kw)
    x2 = interpol.regulariser_solve(g.reshape(2, 1, *g.shape[1:]), h.reshape(2, 1, *h.shape[1:]), **kw)
    assert torch.equal(x2.reshape(x.shape), x)
    assert torch.equal(interpol.regulariser_solve(g[1], h[1], **kw), x[1])
