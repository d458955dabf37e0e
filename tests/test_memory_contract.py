"""The memory contract of the HIP library (MI355X): every case runs with POISONED outputs and workspaces, GUARDED inputs and
GUARDED outputs at once (tests/memguard.py installed as `interpol._hip._empty`), and then asserts

  * every output the library allocated is fully written (no NaN / sentinel left: an element a kernel never wrote, an
    accumulator it did not zero, or a value computed from memory outside an input),
  * every guard byte around every input, output and workspace still holds poison,
  * the values meet the bar the project states elsewhere: float32 rtol 1e-5 + atol 1e-5 max|ref| against the C oracle, float64
    1e-11, 16-bit outputs half an ulp of the format + the float32 bar (tests/storage_contract.py; float32 outputs of a 16-bit call
    that are not grid gradients, the counts, keep LP_TOL), < 4e-6 relative against FLAG_NO_FASTPATH where the generic
    kernels are the yardstick.

Each route runs once with every base pointer aligned and once with the image, the grid, the values and every output shifted by
one element off 16-byte alignment (16-bit storage: by three elements too).  Workspaces always keep their 256-byte alignment:
the library declines the brick routes otherwise.  Sample grids overhang the lattice (linspace(-2, n + 1, m)), extents are
ragged (no multiple of 16, 14 or 64; innermost extents 1, 2, 3 mod 4), bounds and extrapolation modes rotate over the cases.

Proof that a route engaged
  * brick / owner-computes organisations (FLAG_BINNED_SCATTER, backend.rough_deformations = True, push_bricks, the affine
    reduction): `workspace_was_written()` -- the library changed bytes of the poisoned workspace it was handed;
  * the routed default: the same (the probe of the call writes its verdict there), which proves the workspace entry point ran,
    not which organisation the probe picked;
  * LDS tiles: the hand-back mode is pinned ("never" / "always"), so a tile kernel serves the call whatever ran before.
NO PROOF (interpol_kernel_name answers "generic" for every problem, so static dispatch cannot be read back):
  FLAG_FORCE_TILED / natural tiles / the class-sorted scatter (debug bits), float64 push tiles, 16-bit tiles, 1-D push tiles,
  resample1d, pull_labels, the out-of-place prefilter: these are reached by the flags and shapes of the existing tests named
  next to each case, with no read-back.
"""
import contextlib

import numpy as np
import pytest
import torch

import golden_util as G
import interpol
import memguard as M
import storage_contract as SC
from interpol import _hip, backend
from oracle import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NF, TILED, BINNED, SERIAL = _hip.FLAG_NO_FASTPATH, _hip.FLAG_FORCE_TILED, _hip.FLAG_BINNED_SCATTER, _hip.FLAG_SERIAL_ITEMS
NATURAL = TILED | (32 << 8)              # test_golden_mid_fp32: natural-order tiles
SORTED_SCATTER = 128 << 8                # test_golden_mid_fp32: class-sorted scatter
ISHAPE, OSHAPE = (41, 33, 51), (37, 45, 29)
LP_TOL = {torch.bfloat16: 1e-2, torch.float16: 2e-3}
ALIGNS = [0, 1]
STORAGE_ALIGNS = [(torch.float32, 0), (torch.float32, 1)] + [(dt, m) for dt in (torch.bfloat16, torch.float16) for m in (0, 1, 3)]   # (three elements off: the 16-bit types only)
_REF = {}


def _cached(key, make):
    """The reference of a case: computed once, shared by the alignments / variants, never modified."""
    if key not in _REF:
        oracle.set_threads(8)
        try:
            _REF[key] = make()
        finally:
            oracle.set_threads(1)
    return _REF[key]


def _grid(gen, B, lattice, samples, sigma, dtype=torch.float32):
    """Overhanging sample grid; coordinates within 1e-3 of a mask threshold of nd.py:10-27 are moved off it (float32 and float64
    round the threshold differently: see test_sorted_tiles_mixed_orders_against_the_oracle)."""
    dim = len(lattice)
    lin = [torch.linspace(-2, n + 1, m, dtype=dtype) for n, m in zip(lattice, samples)]
    grid = torch.stack(torch.meshgrid(*lin, indexing="ij"), -1)[None] + sigma * torch.randn([B, *samples, dim], generator=gen, dtype=dtype)
    grid = grid.expand(B, *samples, dim).clone()
    for d, n in enumerate(lattice):
        for thr in (-0.55, -0.05, n - 1 + 0.05, n - 1 + 0.55):
            near = (grid[..., d] - thr).abs() < 1e-3
            grid[..., d] = torch.where(near, grid[..., d] + 4e-3, grid[..., d])
    return grid.contiguous()


def _problem(seed, C, sigma, lattice=ISHAPE, samples=OSHAPE, B=2, dtype=torch.float32):
    """vol, gvo on the lattice; src on the sample grid; grid."""
    gen = torch.Generator().manual_seed(seed)
    vol = torch.randn([B, C, *lattice], generator=gen, dtype=dtype)
    src = torch.randn([B, C, *samples], generator=gen, dtype=dtype)
    gvo = torch.randn([B, C, *lattice], generator=gen, dtype=dtype)
    return vol, src, gvo, _grid(gen, B, lattice, samples, sigma, dtype)


def _bounds(i, dim=3):
    return [i % 7, (i + 3) % 7, (i + 5) % 7][:dim]      # mixed per dim, as the oracle tests of the routed operators


class _Env:
    def __init__(self, seam, misalign):
        self.seam, self.misalign, self.inputs = seam, misalign, []

    def put(self, t, dtype=None):
        t = t if dtype is None else t.to(dtype)
        g = M.place(t, DEV, self.misalign)
        self.inputs.append(g)
        return g

    def mark(self):
        return len(self.seam.records)

    def workspace_written_since(self, mark):
        return any(bool((g.interior_bytes() != g.poison).any()) for g in self.seam.records[mark:] if g.workspace and g.tensor.numel())


@contextlib.contextmanager
def contract(monkeypatch, misalign=0, what=""):
    """Poisoned outputs + workspaces, guarded inputs.  On exit: every output fully written, every guard intact."""
    with M.installed(_hip, misalign, monkeypatch) as seam:
        env = _Env(seam, misalign)
        yield env
        torch.cuda.synchronize()
        assert len(seam.outputs()) > 0, "nothing was allocated through the seam"
        for i, g in enumerate(seam.outputs()):
            M.assert_fully_written(g.tensor, None, "%s output %d %s" % (what, i, list(g.tensor.shape)))
            assert g.tensor.data_ptr() % 16 == (misalign * g.tensor.element_size()) % 16
        seam.assert_guards_intact(what)
        for t in env.inputs:
            M.assert_guard_intact(t, "%s input %s" % (what, list(t.shape)))


def _close(got, want, what, tol=1e-5):
    if got.dtype in LP_TOL:                 # a 16-bit output: one rounding of float32 math (tests/storage_contract.py), whatever `tol`
        r = SC.ratio(got.detach().double().cpu().numpy(), want, got.dtype)
        print(what, "storage bar ratio %.3g" % r)
        assert r <= 1.0, (what, r)
        return
    got = got.detach().cpu().numpy()
    want = np.asarray(want)
    print(what, "rel err %.3g" % G.rel_err(got, want))
    G.assert_close(got, want, rtol=tol, atol_rel=tol, what=what)


def _same(fast, slow, tol, what):
    scale = max(float(slow.abs().max()), 1e-30)
    err = float((fast - slow).abs().max()) / scale
    print(what, "vs generic %.3g" % err)
    assert err < tol, (what, err)


@pytest.fixture
def pinned_handback():
    prev = []

    def pin(mode):
        prev.append(_hip.set_handback(mode))
    yield pin
    if prev:
        _hip.set_handback(prev[0])


@pytest.fixture
def routing():
    prev = backend.rough_deformations
    yield
    backend.rough_deformations = prev


def _oracle_all(vol, src, gvo, grid, lattice, b, o, ex, ops):
    v, s, gv, g = vol.double().numpy(), src.double().numpy(), gvo.double().numpy(), grid.double().numpy()
    r = {}
    if "pull" in ops: r["pull"] = oracle.grid_pull(v, g, b, o, ex)
    if "grad" in ops: r["grad"] = oracle.grid_grad(v, g, b, o, ex)
    if "hess" in ops: r["hess"] = oracle.grid_hess(v, g, b, o, ex)
    if "push" in ops: r["push"] = oracle.grid_push(s, g, list(lattice), b, o, ex)
    if "count" in ops: r["count"] = oracle.grid_count(g, list(lattice), b, o, ex)
    if "pushgrad" in ops:
        r["pushgrad"] = oracle.grid_pushgrad(np.repeat(s[..., None], len(lattice), -1) * np.arange(1, len(lattice) + 1), g, list(lattice), b, o, ex)
    if "pullbwd" in ops: r["pullbwd"] = oracle.grid_pull_backward(s, v, g, b, o, ex)
    if "pushbwd" in ops: r["pushbwd"] = oracle.grid_push_backward(gv, s, g, b, o, ex)
    if "countbwd" in ops: r["countbwd"] = oracle.grid_count_backward(gv[:, :1], g, b, o, ex)
    return {k: (tuple(np.asarray(x) for x in v_) if isinstance(v_, tuple) else np.asarray(v_)) for k, v_ in r.items()}


def _run_ops(env, ref, vol, src, gvo, grid, lattice, b, o, ex, flags, what, tol=1e-5, dtype=None, scatter_flags=None, expect_ws=None):
    """Every operator present in `ref`, through `_hip` with `flags`, on guarded inputs."""
    sflags = flags if scatter_flags is None else scatter_flags
    C = vol.shape[1]
    vd, sd, gvd, gd = env.put(vol, dtype), env.put(src, dtype), env.put(gvo, dtype), env.put(grid)
    m0 = env.mark()
    for op in ("pull", "grad", "hess"):
        if op in ref:
            _close(_hip.gather(op, vd, gd, b, o, ex, flags=flags), ref[op], (op,) + what, tol)
    if "push" in ref:
        _close(_hip.scatter("push", sd, gd, list(lattice), b, o, ex, flags=sflags), ref["push"], ("push",) + what, tol)
    if "count" in ref:
        _close(_hip.scatter("count", None, gd, list(lattice), b, o, ex, flags=sflags), ref["count"], ("count",) + what, tol)
    if "push" in ref and "count" in ref:
        both = _hip.scatter("push", sd, gd, list(lattice), b, o, ex, flags=sflags, with_count=True)
        _close(both[:, :C], ref["push"], ("push+count",) + what, tol)
        _close(both[:, C:], ref["count"], ("push+count: count",) + what, tol)
    if "pushgrad" in ref:
        dim = len(lattice)
        sg = env.put(src[..., None] * torch.arange(1, dim + 1, dtype=src.dtype), dtype)
        _close(_hip.scatter("pushgrad", sg, gd, list(lattice), b, o, ex, flags=sflags), ref["pushgrad"], ("pushgrad",) + what, tol)
    if "pullbwd" in ref:
        gi, gg = _hip.pull_backward(sd, vd, gd, b, o, ex, True, True, flags=flags)
        _close(gi, ref["pullbwd"][0], ("pull bwd image",) + what, tol)
        _close(gg, ref["pullbwd"][1], ("pull bwd grid",) + what, 1e-5)
        _close(_hip.pull_backward(sd, vd, gd, b, o, ex, False, True, flags=flags)[1], ref["pullbwd"][1], ("pull bwd grid only",) + what, 1e-5)
    if "pushbwd" in ref:
        pi, pg = _hip.push_backward(gvd, sd, gd, b, o, ex, True, True, flags=flags)
        _close(pi, ref["pushbwd"][0], ("push bwd values",) + what, tol)
        _close(pg, ref["pushbwd"][1], ("push bwd grid",) + what, 1e-5)
    if "countbwd" in ref:
        g1 = env.put(gvo[:, :1].contiguous(), dtype)
        _close(_hip.push_backward(g1, None, gd, b, o, ex, False, True, flags=flags)[1], ref["countbwd"], ("count bwd",) + what, 1e-5)
    if expect_ws:
        assert env.workspace_written_since(m0), ("no workspace was written: the organisation did not run",) + what


ALL_OPS = ("pull", "grad", "hess", "push", "count", "pushgrad", "pullbwd", "pushbwd", "countbwd")
FWD_BWD = ("pull", "grad", "push", "count", "pullbwd", "pushbwd")


# ---- 3-D float32 ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("misalign", ALIGNS)
@pytest.mark.parametrize("order", [0, 3, 7])
def test_generic_kernels(order, misalign, monkeypatch):
    """FLAG_NO_FASTPATH: every operator and both backward passes (test_against_oracle_medium)."""
    i = order % 7
    b, o, ex = _bounds(i), [order] * 3, i % 3
    vol, src, gvo, grid = _problem(10 + order, 2, 2.0)
    ref = _cached(("generic", order), lambda: _oracle_all(vol, src, gvo, grid, ISHAPE, b, o, ex, ALL_OPS))
    with contract(monkeypatch, misalign, "generic") as env:
        _run_ops(env, ref, vol, src, gvo, grid, ISHAPE, b, o, ex, NF, ("generic", order, b, ex, misalign))


@pytest.mark.parametrize("misalign", ALIGNS)
@pytest.mark.parametrize("variant,flags,mode", [("force_tiled", TILED, "never"), ("natural", NATURAL, "always")])
@pytest.mark.parametrize("order", [1, 3, 5, 7])
def test_lds_tiles(order, variant, flags, mode, misalign, monkeypatch, pinned_handback):
    """FLAG_FORCE_TILED and the natural-order tiles (test_tiled_gather_matches_generic, test_golden_mid_fp32), hand-back pinned."""
    pinned_handback(mode)
    i = order + 1
    b, o, ex = _bounds(i), [order] * 3, i % 3
    vol, src, gvo, grid = _problem(20 + order, 3, 2.0)
    ref = _cached(("tiles", order), lambda: _oracle_all(vol, src, gvo, grid, ISHAPE, b, o, ex, FWD_BWD))
    with contract(monkeypatch, misalign, variant) as env:
        _run_ops(env, ref, vol, src, gvo, grid, ISHAPE, b, o, ex, flags, (variant, order, b, ex, misalign))


@pytest.mark.parametrize("misalign", ALIGNS)
@pytest.mark.parametrize("orders", [[1, 1, 1], [2, 2, 2], [3, 3, 3], [1, 2, 3]], ids=["1", "2", "3", "mixed"])
def test_class_sorted_tiles(orders, misalign, monkeypatch):
    """The class-sorted default under a smooth field (sigma = 0.7: test_sorted_tiles_mixed_orders_against_the_oracle) and the class-sorted
    scatter (debug bit 128: test_golden_mid_fp32)."""
    i = sum(orders)
    b, ex = _bounds(i), i % 3
    vol, src, gvo, grid = _problem(30 + i, 2, 0.7)
    ref = _cached(("sorted", tuple(orders)), lambda: _oracle_all(vol, src, gvo, grid, ISHAPE, b, orders, ex, FWD_BWD + ("countbwd",)))
    with contract(monkeypatch, misalign, "sorted") as env:
        _run_ops(env, ref, vol, src, gvo, grid, ISHAPE, b, orders, ex, 0, ("sorted", orders, b, ex, misalign), scatter_flags=SORTED_SCATTER)


@pytest.mark.parametrize("misalign", ALIGNS)
@pytest.mark.parametrize("serial", [0, SERIAL], ids=["chains", "serial"])
@pytest.mark.parametrize("sigma", [0.0, 7.0])
def test_owner_computes_and_bricks_of_the_image(sigma, serial, misalign, monkeypatch):
    """FLAG_BINNED_SCATTER (owner-computes push / count, bricks of the image for pull, grad and the grid gradients) and the routed
    default: test_binned_scatter_rough_deformation_and_modes, test_routed_pull_bricks_of_the_image_against_oracle,
    test_routed_push_and_count_backward_against_oracle, test_push_item_chains."""
    for order in (3, 2):
        i = order + int(sigma)
        b, o, ex = _bounds(i), [order] * 3, i % 3
        vol, src, gvo, grid = _problem(40 + i, 2, sigma)
        ref = _cached(("owner", order, sigma), lambda: _oracle_all(vol, src, gvo, grid, ISHAPE, b, o, ex, FWD_BWD + ("countbwd",)))
        for name, fl in (("bricks", BINNED), ("routed", 0)):
            with contract(monkeypatch, misalign, name) as env:
                _run_ops(env, ref, vol, src, gvo, grid, ISHAPE, b, o, ex, fl, (name, order, sigma, b, ex, serial, misalign),
                         scatter_flags=(fl | serial) if (fl or not serial) else (_hip.FLAG_AUTO_SCATTER | serial), expect_ws=True)
                assert env.seam.workspace_was_written()


@pytest.mark.parametrize("misalign", ALIGNS)
@pytest.mark.parametrize("flags", [0, BINNED], ids=["routed", "bricks"])
@pytest.mark.parametrize("order", [4, 5, 6, 7])
def test_gather5_gather7(order, flags, misalign, monkeypatch):
    """Orders 4 - 7 through gather5.hip / gather7.hip (test_orders_4_and_5_push_and_count_through_bricks_of_the_target,
    test_orders_4_and_5_through_bricks_of_the_image_against_oracle)."""
    i = order + 2
    b, o, ex = _bounds(i), [order] * 3, i % 3
    vol, src, gvo, grid = _problem(50 + order, 2, 5.0)
    ref = _cached(("g57", order), lambda: _oracle_all(vol, src, gvo, grid, ISHAPE, b, o, ex, ("pull", "grad", "push", "count")))
    with contract(monkeypatch, misalign, "gather5/7") as env:
        _run_ops(env, ref, vol, src, gvo, grid, ISHAPE, b, o, ex, flags, ("gather57", order, flags, b, ex, misalign), expect_ws=True)


@pytest.mark.parametrize("misalign", ALIGNS)
def test_push_bricks(misalign, monkeypatch):
    """_hip.push_bricks at zoom 4 (test_push_bricks_matches_push): push and push + count."""
    gen = torch.Generator().manual_seed(60)
    sshape = (21, 26, 19)
    tshape = [int(n * 4.0) + 5 for n in sshape]            # 89 x 109 x 81
    lin = [torch.arange(n, dtype=torch.float32) * 4.0 for n in sshape]
    grid = (torch.stack(torch.meshgrid(*lin, indexing="ij"), -1)[None] + 1.7 * torch.randn([2, *sshape, 3], generator=gen)).contiguous()
    src = torch.randn([2, 3, *sshape], generator=gen)
    b, o = [1, 4, 6], [3] * 3

    def make():
        oracle_p = [np.asarray(oracle.grid_push(src.double().numpy(), grid.double().numpy(), tshape, b, o, ex)) for ex in (0, 1, 2)]
        oracle_c = [np.asarray(oracle.grid_count(grid.double().numpy(), tshape, b, o, ex)) for ex in (0, 1, 2)]
        return oracle_p, oracle_c
    want_p, want_c = _cached("push_bricks", make)
    with contract(monkeypatch, misalign, "push_bricks") as env:
        sd, gd = env.put(src), env.put(grid)
        for ex in (0, 1, 2):
            _close(_hip.push_bricks(sd, gd, tshape, b, o, ex), want_p[ex], ("push_bricks", ex, misalign))
            both = _hip.push_bricks(sd, gd, tshape, b, o, ex, with_count=True)
            _close(both[:, :3], want_p[ex], ("push_bricks+count", ex, misalign))
            _close(both[:, 3:], want_c[ex], ("push_bricks+count: count", ex, misalign))
        assert env.seam.workspace_was_written()


# ---- float64, 16-bit storage ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("misalign", ALIGNS)
def test_float64_push_tiles(misalign, monkeypatch):
    """csrc/push_f64.hip (>= 4096 samples): push, count, push + count, the image gradient of pull backward at 1e-11
    (test_float64_push_tiles_against_oracle_and_generic)."""
    for k, (orders, sigma) in enumerate((([3, 3, 3], 2.5), ([1, 3, 2], 0.0), ([2, 0, 3], 7.0))):
        b, ex = _bounds(k + 4), k % 3
        vol, src, gvo, grid = _problem(70 + k, 2, sigma, dtype=torch.float64)
        ref = _cached(("f64", k), lambda: _oracle_all(vol, src, gvo, grid, ISHAPE, b, orders, ex, ("push", "count", "pullbwd")))
        with contract(monkeypatch, misalign, "f64") as env:
            sd, vd, gd = env.put(src), env.put(vol), env.put(grid)
            both = _hip.scatter("push", sd, gd, list(ISHAPE), b, orders, ex, with_count=True)
            assert G.rel_err(both[:, :2].cpu().numpy(), ref["push"]) < 1e-11, ("push", orders, b, ex)
            assert G.rel_err(both[:, 2:].cpu().numpy(), ref["count"]) < 1e-11, ("count channel", orders, b, ex)
            assert G.rel_err(_hip.scatter("count", None, gd, list(ISHAPE), b, orders, ex).cpu().numpy(), ref["count"]) < 1e-11, ("count", orders, b, ex)
            gi, gg = _hip.pull_backward(sd, vd, gd, b, orders, ex, True, True)
            assert G.rel_err(gi.cpu().numpy(), ref["pullbwd"][0]) < 1e-11 and G.rel_err(gg.cpu().numpy(), ref["pullbwd"][1]) < 1e-11, ("pull bwd", orders, b, ex)


@pytest.mark.parametrize("misalign", [0, 1, 3])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_low_precision_storage_3d(dtype, misalign, monkeypatch, pinned_handback):
    """bf16 / f16 storage in 3-D: the tiles (cubic), the routed trilinear pull, the fp32 scratch accumulator of push and of the image
    gradient of pull backward (test_tiled_low_precision_storage_matches_generic, test_trilinear_pull_router)."""
    pinned_handback("never")
    tol = LP_TOL[dtype]
    for order, fl in ((3, TILED), (1, 0)):
        b, o, ex = _bounds(order + 1), [order] * 3, order % 3
        vol, src, gvo, grid = _problem(80 + order, 3, 1.5)
        vol, src = vol.to(dtype).float(), src.to(dtype).float()            # the oracle sees the stored values
        ref = _cached(("lowp", str(dtype), order), lambda: _oracle_all(vol, src, gvo, grid, ISHAPE, b, o, ex, ("pull", "push", "pullbwd")))
        with contract(monkeypatch, misalign, "lowp") as env:
            vd, sd, gd = env.put(vol, dtype), env.put(src, dtype), env.put(grid)
            got = _hip.gather("pull", vd, gd, b, o, ex, flags=fl)
            assert got.dtype == dtype
            _close(got, ref["pull"], ("pull", dtype, order, misalign), tol)
            got = _hip.scatter("push", sd, gd, list(ISHAPE), b, o, ex, flags=fl)
            assert got.dtype == dtype
            _close(got, ref["push"], ("push", dtype, order, misalign), tol)
            gi = _hip.pull_backward(sd, vd, gd, b, o, ex, True, False, flags=fl)[0]
            assert gi.dtype == dtype
            _close(gi, ref["pullbwd"][0], ("pull bwd image", dtype, order, misalign), tol)
            assert all(g.tensor.data_ptr() % 256 == 0 for g in env.seam.workspaces())


# ---- 2-D, 1-D ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sigma,rough", [(0.0, None), (12.0, True)], ids=["lean_tiles", "bricks"])
@pytest.mark.parametrize("dtype,misalign", STORAGE_ALIGNS)
def test_two_d(dtype, misalign, sigma, rough, monkeypatch, routing):
    """Everything test_two_d_operators_through_bricks calls, on (90, 77) <- (85, 101): the lean tiles behind the default at sigma = 0
    and the bricks (backend.rough_deformations = True) at sigma = 12; 16-bit storage as test_two_d_bricks_low_precision_storage."""
    lattice, samples = (90, 77), (85, 101)
    tol = LP_TOL.get(dtype, 1e-5)
    for k in range(2):
        i = k + int(sigma) + (0 if dtype == torch.float32 else 3)
        o = [1 + i % 3, 1 + (i // 2) % 3]
        b, ex, C = [i % 7, (i + 3) % 7], (i + o[0]) % 3, 1 + (2 * i) % 5
        vol, src, gvo, grid = _problem(90 + i, C, sigma, lattice, samples)
        if dtype != torch.float32:
            vol, src, gvo = (t.to(dtype).float() for t in (vol, src, gvo))
        ref = _cached(("2d", str(dtype), sigma, k), lambda: _oracle_all(vol, src, gvo, grid, lattice, b, o, ex, ("pull", "push", "count", "pullbwd", "pushbwd", "countbwd")))
        backend.rough_deformations = rough
        with contract(monkeypatch, misalign, "2d") as env:
            _run_ops(env, ref, vol, src, gvo, grid, lattice, b, o, ex, 0, ("2d", dtype, sigma, o, b, ex, C, misalign), tol=tol,
                     dtype=None if dtype == torch.float32 else dtype, expect_ws=bool(rough))


@pytest.mark.parametrize("misalign", ALIGNS)
@pytest.mark.parametrize("flags", [0, NF], ids=["tiles", "generic"])
@pytest.mark.parametrize("order", [1, 3, 7])
def test_push1d(order, flags, misalign, monkeypatch):
    """1-D push / count: the LDS tiles of csrc/push1d.hip behind the default and the generic kernel (test_push1d_tiles_against_the_oracle)."""
    gen = torch.Generator().manual_seed(100 + order)
    for k, (n_in, n_out, zoom, sigma) in enumerate(((5001, 5003, 1.0, 2.0), (4099, 901, 0.22, 3.0))):
        b, ex, C = [(order + 3 * k) % 7], (order + k) % 3, 1 + (order + k) % 3
        src = torch.randn([3, C, n_in], generator=gen)
        grid = (torch.arange(n_in, dtype=torch.float32) * zoom - 2 + sigma * torch.randn([3, n_in], generator=gen))[..., None].contiguous()
        for thr in (-0.55, -0.05, n_out - 1 + 0.05, n_out - 1 + 0.55):
            grid = torch.where((grid - thr).abs() < 1e-3, grid + 4e-3, grid)
        ref = _cached(("1d", order, k), lambda: (np.asarray(oracle.grid_push(src.double(), grid.double(), [n_out], b, [order], ex)),
                                                 np.asarray(oracle.grid_count(grid.double(), [n_out], b, [order], ex))))
        with contract(monkeypatch, misalign, "push1d") as env:
            sd, gd = env.put(src), env.put(grid)
            both = _hip.scatter("push", sd, gd, [n_out], b, [order], ex, flags=flags, with_count=True)
            _close(both[:, :C], ref[0], ("push1d", order, k, flags, misalign))
            _close(both[:, C:], ref[1], ("push1d count channel", order, k, flags, misalign))
            _close(_hip.scatter("push", sd, gd, [n_out], b, [order], ex, flags=flags), ref[0], ("push1d alone", order, k, flags, misalign))
            _close(_hip.scatter("count", None, gd, [n_out], b, [order], ex, flags=flags), ref[1], ("count1d", order, k, flags, misalign))


# ---- other entry points --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("misalign", ALIGNS)
@pytest.mark.parametrize("order", [1, 3, 7])
def test_resample1d(order, misalign, monkeypatch):
    """interpol_resample_1d forward and adjoint (test_resample1d_passes): forward == the generic 1-D pull of the same line at 1e-12
    (float64) / 1e-5 (float32), adjoint == exact transpose."""
    gen = torch.Generator().manual_seed(order)
    x = torch.randn([3, 13, 5, 11], generator=gen, dtype=torch.float64)
    mode = 1 if order == 1 else 0
    for dim, n in ((1, 13), (3, 11), (2, 5)):
        lin = torch.linspace(-2.5, n + 1.5, 17, dtype=torch.float64) + 0.05 * torch.randn(17, generator=gen, dtype=torch.float64)
        bound, ex = (order + dim) % 7, dim % 3
        y = torch.randn([17 if d == dim else s for d, s in enumerate(x.shape)], generator=gen, dtype=torch.float64)
        xm = x.to(DEV).movedim(dim, -1).reshape(-1, 1, n)
        ref = _hip.gather("pull", xm, lin.to(DEV).reshape(1, -1, 1), [bound], [order], ex, flags=NF)
        ref = ref.reshape(*x.movedim(dim, -1).shape[:-1], 17).movedim(-1, dim)
        with contract(monkeypatch, misalign, "resample1d") as env:
            xd, ld, yd = env.put(x), env.put(lin), env.put(y)
            got = _hip.resample1d(xd, ld, dim, order, bound, ex, mode)
            _same(got, ref, 1e-12, ("fwd", order, dim, bound, ex, misalign))
            adj = _hip.resample1d(yd, ld, dim, order, bound, ex, mode, adjoint=True, n_lattice=n)
            lhs, rhs = float((got * yd).sum()), float((xd * adj).sum())
            assert abs(lhs - rhs) <= 1e-10 * max(abs(lhs), abs(rhs), 1.0), ("adjoint", order, dim, bound, ex)
            x32, l32 = env.put(x.float()), env.put(lin.float())
            got32 = _hip.resample1d(x32, l32, dim, order, bound, ex, mode)
            want32 = _hip.resample1d(x.float().double().to(DEV), lin.float().double().to(DEV), dim, order, bound, ex, mode)
            _same(got32.double(), want32, 1e-5, ("f32", order, dim, misalign))


@pytest.mark.parametrize("misalign", ALIGNS)
@pytest.mark.parametrize("dim,order", [(3, 3), (3, 1), (2, 3), (1, 0)])
def test_pull_labels(dim, order, misalign, monkeypatch):
    """interpol_pull_labels (test_label_map_fused_matches_loop): int32 output poisoned with a sentinel no label equals; against the
    loop over labels built from the generic float pull, flips tolerated at numerical ties only (< 2e-4 of the samples)."""
    gen = torch.Generator().manual_seed(dim * 7 + order)
    ishape, oshape = (23, 31, 19)[:dim], (41, 27, 33)[:dim]
    lab = torch.randint(0, 37, [2, 2, *ishape], generator=gen).to(torch.int32)
    grid = _grid(gen, 2, ishape, oshape, 1.3)
    for bound, ex in ((0, 0), (3, 1), (6, 2)):
        out = torch.zeros([2, 2, *oshape], dtype=torch.long, device=DEV)
        pmax = torch.zeros(out.shape, device=DEV)
        for l in lab.unique():
            soft = _hip.gather("pull", (lab == l).float().to(DEV), grid.to(DEV), [bound] * dim, [order] * dim, ex, flags=NF)
            out[soft > pmax] = int(l)
            pmax = torch.max(pmax, soft)
        with contract(monkeypatch, misalign, "labels") as env:
            fused = _hip.pull_labels(env.put(lab), env.put(grid), [bound] * dim, [order] * dim, ex)
            assert fused.dtype == torch.int32
            assert int((fused == M.LABEL_POISON).sum()) == 0
            mism = float((fused.long() != out).float().mean())
            assert mism < 2e-4, (dim, order, bound, ex, mism)


@pytest.mark.parametrize("dtype,misalign", STORAGE_ALIGNS + [(torch.float64, 0), (torch.float64, 1)])
def test_prefilter_out_of_place(dtype, misalign):
    """spline_filter_(dst, src=) (test_prefilter_out_of_place_reads_source_writes_result): a poisoned, guarded destination; the
    source untouched, the result bit-identical to the in-place call."""
    gen = torch.Generator().manual_seed(77)
    for shape, dim in (([6, 257, 1], 1), ([2, 513, 41], 1), ([3, 101, 7], 1), ([2, 3, 67, 255], 2), ([2, 65, 33], 1)):
        x = torch.randn(shape, generator=gen).to(dtype)
        for order in (2, 3, 5):
            src = M.place(x, DEV, misalign)
            dst = M.guarded(shape, dtype, DEV, misalign)
            ref = _hip.spline_filter_(x.to(DEV).clone(), 3, order, dim)
            _hip.spline_filter_(dst, 3, order, dim, src=src)
            torch.cuda.synchronize()
            M.assert_fully_written(dst, None, ("prefilter", shape, dtype, order))
            M.assert_guard_intact(dst, "prefilter dst")
            M.assert_guard_intact(src, "prefilter src")
            assert torch.equal(src, x.to(DEV)) and torch.equal(dst, ref), (shape, dtype, order, misalign)


@pytest.mark.parametrize("misalign", ALIGNS)
@pytest.mark.parametrize("dim", [2, 3])
def test_affine_backward(dim, misalign, monkeypatch):
    """The matrix gradient of an AffineGrid (csrc/affine_grad.hip; test_affine_grad_mat_matches_the_c_oracle): its workspace of
    per-workgroup partial sums poisoned, the (D, D+1) result guarded; float32 at that test's allowance."""
    import test_affine_grad_gpu as AG
    vol, src, shp, oshp = AG._inputs(dim, torch.float64, 190 + dim)
    b, o, ex = [3] * dim, [3] * dim, 1

    def make():
        dn = interpol.affine_grid(AG._mat(dim, torch.float64), oshp)[None].expand(2, *oshp, dim).contiguous().numpy()
        _, gg = oracle.grid_pull_backward(src.numpy(), vol.numpy(), dn, b, o, ex)
        gg = np.asarray(gg).reshape(2, -1, dim)
        idx = AG._index(oshp, device="cpu").numpy()
        return (torch.as_tensor(np.einsum("bnd,ne->de", gg, idx)),
                torch.as_tensor(np.einsum("nd,ne->de", (np.abs(gg) + np.abs(gg).max(axis=(0, 1), keepdims=True)).sum(0), idx)))
    want, allow = _cached(("affine", dim), make)
    for dtype in (torch.float64, torch.float32):
        lazy = interpol.AffineGrid(AG._mat(dim, dtype), oshp).to(DEV)
        with contract(monkeypatch, misalign, "affine") as env:
            got = _hip.affine_pull_backward(env.put(src.to(dtype)), env.put(vol.to(dtype)), lazy, b, o, ex)
            AG._check(got.cpu(), want, allow, AG.TOL[dtype], ("affine pull", dim, str(dtype), misalign))
            pg = _hip.affine_push_backward(env.put(vol.to(dtype)), env.put(src.to(dtype)), lazy, b, o, ex)
            assert bool(torch.isfinite(pg).all())
            assert env.seam.workspace_was_written()


# ---- many tiles per workgroup (ADVICE: ops_tiled.hip, "output entries never written, or a fault, under rough fields") -------------------

MANY = (112, 96, 104)


def _many_problem(C):
    gen = torch.Generator().manual_seed(900 + C)
    ident = interpol.identity_grid(MANY)[None]
    vol = torch.randn([2, C, *MANY], generator=gen)
    src = torch.randn([2, C, *MANY], generator=gen)
    grid = (ident + 9.0 * torch.randn([2, *MANY, 3], generator=gen)).contiguous()
    return vol, src, grid


def _many_reference(C):
    def make():
        vol, src, grid = (t.to(DEV) for t in _many_problem(C))
        b, o = [3] * 3, [3] * 3
        r = dict(pull=_hip.gather("pull", vol, grid, b, o, 1, flags=NF).cpu(),
                 push=_hip.scatter("push", src, grid, list(MANY), b, o, 1, flags=NF).cpu())
        gi, gg = _hip.pull_backward(src, vol, grid, b, o, 1, True, True, flags=NF)
        r["gvol"], r["ggrid"] = gi.cpu(), gg.cpu()
        return r
    return _cached(("many", C), make)


@pytest.mark.parametrize("mode", ["always", "never"])
@pytest.mark.parametrize("C", [1, 3])
def test_many_tiles_rough_field_covers_every_output(C, mode, monkeypatch, pinned_handback):
    """gather_tiled, push_tiled and pullbwd_tiled where a workgroup serves several tiles of a rough field (112 x 96 x 104, sigma = 9):
    poisoned outputs, hand-back always / never, one and three channels, one and both gradients; full coverage and the generic kernels'
    values at 4e-6."""
    ref = {k: v.to(DEV) for k, v in _many_reference(C).items()}
    pinned_handback(mode)
    vol, src, grid = _many_problem(C)
    b, o = [3] * 3, [3] * 3
    with contract(monkeypatch, 0, "many tiles") as env:
        vd, sd, gd = env.put(vol), env.put(src), env.put(grid)
        _same(_hip.gather("pull", vd, gd, b, o, 1, flags=TILED), ref["pull"], 4e-6, ("gather_tiled", C, mode))
        _same(_hip.scatter("push", sd, gd, list(MANY), b, o, 1, flags=TILED), ref["push"], 4e-6, ("push_tiled", C, mode))
        for nv, ng in ((True, True), (False, True), (True, False)):
            gi, gg = _hip.pull_backward(sd, vd, gd, b, o, 1, nv, ng, flags=TILED)
            if nv:
                _same(gi, ref["gvol"], 4e-6, ("pullbwd_tiled image", C, mode, nv, ng))
            if ng:
                _same(gg, ref["ggrid"], 4e-6, ("pullbwd_tiled grid", C, mode, nv, ng))


# ---- zero-fill -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("misalign", [0, 1, 2, 3])
def test_zero_fill_of_ragged_misaligned_targets(dtype, misalign, monkeypatch):
    """zero_async (csrc/abi.hip: head bytes, 16-byte body, tail bytes) through scatter(..., out=guarded(...)): every sample is outside
    the field of view and extrapolate = 0, so the whole target must be exactly 0 -- also a target smaller than 16 bytes -- and
    nothing beyond it may be touched."""
    gen = torch.Generator().manual_seed(3)
    for shape in ([3], [1], [5], [7, 3], [3, 3, 3], [13, 11], [5, 7, 9], [33], [4, 4, 4]):
        dim = len(shape)
        grid = (-100.0 - 50.0 * torch.rand([1, *[5] * dim, dim], generator=gen)).to(dtype)
        src = torch.randn([1, 1, *[5] * dim], generator=gen).to(dtype)
        for op in ("push", "count"):
            for fl in (0, NF):
                with M.installed(_hip, 0, monkeypatch) as seam:
                    out = M.guarded([1, 1] + shape, dtype, DEV, misalign)
                    assert out.data_ptr() % 16 == (misalign * out.element_size()) % 16
                    sd, gd = M.place(src, DEV, misalign), M.place(grid, DEV, misalign)
                    got = _hip.scatter(op, sd if op == "push" else None, gd, shape, [0] * dim, [1] * dim, 0, flags=fl, out=out)
                    torch.cuda.synchronize()
                    assert got.data_ptr() == out.data_ptr()
                    assert int((out != 0).sum()) == 0 and M.unwritten(out) == 0, (op, shape, dtype, misalign, fl)
                    M.assert_guard_intact(out, ("zero fill", op, shape, dtype, misalign, fl))
                    seam.assert_guards_intact("zero fill")
