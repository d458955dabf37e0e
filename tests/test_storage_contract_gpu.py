"""bf16 / f16 storage held to its contract ("float32 math, rounded once"): every 16-bit output of every route that takes
16-bit storage lies within  0.5 ulp16 + e32  of the float64 truth of the STORED inputs (tests/storage_contract.py: `bar`), every
float32 output of such a call (grid gradients) within the plain float32 bar  e32 = 1e-5 |want| + 1e-5 max|want|.  Truth is the C
oracle in float64 (oracle/), for resample1d the dense pass matrix of tests/separable_truth.py.

Shapes, route-forcing flags, overhanging grids, rotated bounds / extrapolation modes, the poisoned and guarded buffers and the proofs
of engagement are those of tests/test_memory_contract.py, whose helpers are imported: 3-D (41, 33, 51) sampled at (37, 45, 29), 2-D
(90, 77) <- (85, 101), 1-D 5001 -> 5003 and 4099 -> 901.  Bases are aligned, one element and three elements off 16 bytes in turn.

THE ROUTES THAT TAKE 16-BIT STORAGE (csrc/abi.hip, and the launchers it asks), and how each is reached here
  generic kernels (ops_generic.hpp, *_bf16 / *_f16 of ops_instantiate.inc): pull, grad, push, both backward passes, D = 1, 2, 3
      FLAG_NO_FASTPATH                                                                           test_generic_kernels
  the float32 accumulator of a 16-bit target and its one narrowing (abi.hip: scatter_driver, interpol_pull_backward ->
      launch_narrow_*): under EVERY push and every image gradient below
  3-D LDS tiles (ops_tiled.hip: launch_gather / launch_push / launch_pullbwd / launch_pushbwd, orders 1 - 7)
      FLAG_FORCE_TILED, hand-back "never", and the natural-order tiles (debug bit 32), hand-back "always"; no read-back
                                                                                                 test_lds_tiles
  the routed trilinear pull (abi.hip: linear_routed -> lin_probe, then pull_sorted<T, 1> or the generic kernel)
      flags 0 (the probe's verdict is written to the workspace: proof that the entry point ran) and FLAG_BINNED_SCATTER (the
      class-sorted K = 1 tiles unconditionally)                                                  test_trilinear_pull_router
  class-sorted 3-D tiles (ops_sorted.hip: pull_sorted orders 2, 3 and mixed behind the plain interpol_pull; gradc_sorted for the
      float32 grid gradients; the class-sorted scatter behind debug bit 128)
      flags 0, sigma = 0.7; no read-back                                                         test_class_sorted_tiles
  owner-computes push (push_owner.hip: launch_bin<bf16_t / f16_t>, values binned in their own format, float32 sums)
      FLAG_BINNED_SCATTER and backend.rough_deformations = True, sigma = 0 and 7; workspace_was_written()
                                                                                                 test_owner_computes_push
  lean 2-D tiles (ops_tiled2d.hip) behind the default at sigma = 0, 2-D bricks (scatter2d.hip: gather2d / scatter2d) under
      backend.rough_deformations = True at sigma = 12 (workspace written)                        test_two_d
  1-D push tiles (push1d.hip) behind the default, against the oracle like the generic kernel's flag; no read-back
                                                                                                 test_push1d
  interpol_resample_1d forward (resample1d.hip: launch_k<bf16_t / f16_t, float, float>), one pass per call; no read-back
                                                                                                 test_resample1d_forward
NOT 16-BIT ROUTES (float32 only, by their eligibility tests): the bricks of the image (push_owner.hip: own_gather), gather5.hip /
gather7.hip (orders 4 - 7 through bricks), interpol_push_bricks, the float64 push tiles, pull_labels; hess and pushgrad are computed
in float32 and narrowed by the host.  A 16-bit call with their flags lands on the routes above: orders 4 - 7 under the routed
default and FLAG_BINNED_SCATTER in test_orders_4_to_7_with_the_flags_of_the_float32_bricks.
OUT OF SCOPE: interpol_spline_filter.  Its in-place kernels round after every pass by design (profiles/separable_parity.txt); it
keeps its own bar in tests/test_prefilter_gpu.py.

EDGES: exact ties bit for bit (linear pull at i + 0.5 between adjacent numbers of the format, every route that takes order 1),
order 0 as an exact gather, outputs six decades below max|want|, f16 subnormal results, f16 overflow of a push.

Every comparison prints `STORAGE route operator type ratio ulps` before it asserts: `python tests/storage_contract.py` condenses a
`-s` log into profiles/storage_contract.txt."""
import numpy as np
import pytest
import torch

import separable_truth as ST
import storage_contract as SC
import test_memory_contract as MC
import test_separable_gpu as TS
from interpol import _hip, backend
from oracle import oracle
from test_memory_contract import pinned_handback, routing          # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NF, TILED, BINNED = MC.NF, MC.TILED, MC.BINNED
ISHAPE, OSHAPE = MC.ISHAPE, MC.OSHAPE
L2, S2 = (90, 77), (85, 101)
TYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "f16"]
OPS = ("pull", "grad", "push", "pullbwd", "pushbwd")


class Tally:
    """The comparisons of one case: each prints its figures, `done` asserts them all."""

    def __init__(self, route):
        self.route, self.bad = route, []

    def _note(self, op, dt, r, u, what):
        print("STORAGE %s %s %s %.4f %.4f" % (self.route, op.replace(" ", "_"), dt, r, u))
        if not r <= 1.0:
            self.bad.append((op, dt, round(r, 4), round(u, 4)) + tuple(what))

    def lp(self, got, want, dtype, op, what=()):
        assert got.dtype == dtype, (op, got.dtype)
        g, w = got.detach().double().cpu().numpy(), np.asarray(want, dtype=np.float64)
        self._note(op, SC.name(dtype), SC.ratio(g, w, dtype), SC.ulps(g, w, dtype), what)

    def f32(self, got, want, op, what=()):
        assert got.dtype == torch.float32, (op, got.dtype)
        g, w = got.detach().double().cpu().numpy(), np.asarray(want, dtype=np.float64)
        self._note(op, "f32", SC.f32_ratio(g, w), 0.0, what)

    def done(self):
        assert not self.bad, "%s: outside the bar (operator, type, ratio, ulps, case): %s" % (self.route, self.bad)


def _stored(dtype, *tensors):
    """The values as stored in `dtype`, widened to float32 (exact): what the kernels read and what the oracle is given."""
    return tuple(t.to(dtype).float() for t in tensors)


def _truth(key, vol, src, gvo, grid, lattice, b, o, ex, ops):
    return MC._cached(("storage",) + key, lambda: MC._oracle_all(vol, src, gvo, grid, lattice, b, o, ex, ops))


def _run(env, t, ref, vol, src, gvo, grid, lattice, b, o, ex, flags, dtype, what, scatter_flags=None, with_count=False):
    """Every operator present in `ref` through `_hip` with `flags`, 16-bit storage on guarded inputs."""
    sflags = flags if scatter_flags is None else scatter_flags
    C = vol.shape[1]
    vd, sd, gvd, gd = env.put(vol, dtype), env.put(src, dtype), env.put(gvo, dtype), env.put(grid)
    if "pull" in ref:
        t.lp(_hip.gather("pull", vd, gd, b, o, ex, flags=flags), ref["pull"], dtype, "pull", what)
    if "grad" in ref:
        t.lp(_hip.gather("grad", vd, gd, b, o, ex, flags=flags), ref["grad"], dtype, "grad", what)
    if "push" in ref:
        t.lp(_hip.scatter("push", sd, gd, list(lattice), b, o, ex, flags=sflags), ref["push"], dtype, "push", what)
        if with_count:
            both = _hip.scatter("push", sd, gd, list(lattice), b, o, ex, flags=sflags, with_count=True)
            t.lp(both[:, :C], ref["push"], dtype, "push+count", what)
            t.lp(both[:, C:], ref["count"], dtype, "push+count: count", what)
    if "pullbwd" in ref:
        gi, gg = _hip.pull_backward(sd, vd, gd, b, o, ex, True, True, flags=flags)
        t.lp(gi, ref["pullbwd"][0], dtype, "pullbwd image", what)
        t.f32(gg, ref["pullbwd"][1], "pullbwd grid", what)
        t.lp(_hip.pull_backward(sd, vd, gd, b, o, ex, True, False, flags=flags)[0], ref["pullbwd"][0], dtype, "pullbwd image alone", what)
        t.f32(_hip.pull_backward(sd, vd, gd, b, o, ex, False, True, flags=flags)[1], ref["pullbwd"][1], "pullbwd grid alone", what)
    if "pushbwd" in ref:
        pi, pg = _hip.push_backward(gvd, sd, gd, b, o, ex, True, True, flags=flags)
        t.lp(pi, ref["pushbwd"][0], dtype, "pushbwd values", what)
        t.f32(pg, ref["pushbwd"][1], "pushbwd grid", what)
        t.lp(_hip.push_backward(gvd, sd, gd, b, o, ex, True, False, flags=flags)[0], ref["pushbwd"][0], dtype, "pushbwd values alone", what)


def _case(i):
    """Channels (1 or an odd count) and the misalignment of case i: every pair is met."""
    return (1, 3)[i % 2], (0, 1, 3)[(i // 2) % 3]


# ---- the routes ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", TYPES, ids=IDS)
@pytest.mark.parametrize("order", [1, 3, 7])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_generic_kernels(dim, order, dtype, monkeypatch):
    lattice, samples = {1: ((901,), (4099,)), 2: (L2, S2), 3: (ISHAPE, OSHAPE)}[dim]
    i = dim + order + IDS.index(SC.name(dtype))
    C, misalign = _case(i)
    b, o, ex = MC._bounds(i, dim), [order] * dim, i % 3
    vol, src, gvo, grid = MC._problem(300 + 10 * dim + order, C, 2.0, lattice, samples)
    vol, src, gvo = _stored(dtype, vol, src, gvo)
    ref = _truth(("generic", dim, order, str(dtype)), vol, src, gvo, grid, lattice, b, o, ex, OPS)
    t = Tally("generic_%dd" % dim)
    with MC.contract(monkeypatch, misalign, "generic 16-bit") as env:
        _run(env, t, ref, vol, src, gvo, grid, lattice, b, o, ex, NF, dtype, (order, b, ex, C, misalign))
    t.done()


@pytest.mark.parametrize("dtype", TYPES, ids=IDS)
@pytest.mark.parametrize("variant,flags,mode", [("force_tiled", TILED, "never"), ("natural", MC.NATURAL, "always")])
@pytest.mark.parametrize("order", [1, 3, 5, 7])
def test_lds_tiles(order, variant, flags, mode, dtype, monkeypatch, pinned_handback):
    """(f16: no truth of these cases comes near the end of the format's range -- asserted -- so every order runs in both types.)"""
    pinned_handback(mode)
    i = order + IDS.index(SC.name(dtype)) + (variant == "natural")
    C, misalign = _case(i)
    b, o, ex = MC._bounds(i + 1), [order] * 3, (i + 1) % 3
    vol, src, gvo, grid = MC._problem(320 + order, C, 2.0)
    vol, src, gvo = _stored(dtype, vol, src, gvo)
    ref = _truth(("tiles", order, variant, str(dtype)), vol, src, gvo, grid, ISHAPE, b, o, ex, OPS)
    assert max(float(np.abs(np.asarray(ref[k][0] if isinstance(ref[k], tuple) else ref[k])).max()) for k in ref) < SC.F16_MAX / 4
    t = Tally("lds_tiles_" + variant)
    with MC.contract(monkeypatch, misalign, "tiles 16-bit") as env:
        _run(env, t, ref, vol, src, gvo, grid, ISHAPE, b, o, ex, flags, dtype, (order, b, ex, C, misalign))
    t.done()


@pytest.mark.parametrize("dtype", TYPES, ids=IDS)
@pytest.mark.parametrize("flags", [0, BINNED], ids=["routed", "bricks_flag"])
@pytest.mark.parametrize("order", [4, 5, 6, 7])
def test_orders_4_to_7_with_the_flags_of_the_float32_bricks(order, flags, dtype, monkeypatch):
    """gather5.hip / gather7.hip and the bricks of the image are float32 organisations: a 16-bit call with their flags (the routed
    default, FLAG_BINNED_SCATTER) is served by the tiles and the generic kernels, and meets the same contract there.  (With
    FLAG_BINNED_SCATTER the backward for both gradients used to fail with INTERPOL_E_NULL: the host replaced the float32 accumulator
    of the 16-bit image gradient by the -- empty -- bricks workspace.)"""
    i = order + IDS.index(SC.name(dtype)) + (1 if flags else 0)
    C, misalign = _case(i)
    b, o, ex = MC._bounds(i + 2), [order] * 3, i % 3
    vol, src, gvo, grid = MC._problem(350 + order, C, 5.0)
    vol, src, gvo = _stored(dtype, vol, src, gvo)
    ref = _truth(("g57", order, flags, str(dtype)), vol, src, gvo, grid, ISHAPE, b, o, ex, ("pull", "grad", "push", "pullbwd"))
    t = Tally("orders_4_to_7_" + ("bricks_flag" if flags else "routed"))
    with MC.contract(monkeypatch, misalign, "orders 4 - 7, 16-bit") as env:
        _run(env, t, ref, vol, src, gvo, grid, ISHAPE, b, o, ex, flags, dtype, (order, b, ex, C, misalign))
    t.done()


@pytest.mark.parametrize("dtype", TYPES, ids=IDS)
@pytest.mark.parametrize("sigma", [0.05, 5.0])
def test_trilinear_pull_router(sigma, dtype, monkeypatch):
    i = int(sigma) + IDS.index(SC.name(dtype))
    C, misalign = _case(i)
    b, o, ex = MC._bounds(i + 2), [1] * 3, i % 3
    vol, src, gvo, grid = MC._problem(340 + i, C, sigma)
    vol, = _stored(dtype, vol)
    ref = _truth(("trilinear", sigma, str(dtype)), vol, src, gvo, grid, ISHAPE, b, o, ex, ("pull",))
    for name, fl in (("trilinear_routed", 0), ("trilinear_sorted_tiles", BINNED)):
        t = Tally(name)
        with MC.contract(monkeypatch, misalign, name) as env:
            vd, gd = env.put(vol, dtype), env.put(grid)
            m0 = env.mark()
            t.lp(_hip.gather("pull", vd, gd, b, o, ex, flags=fl), ref["pull"], dtype, "pull", (sigma, b, ex, C, misalign))
            if fl == 0:
                assert env.workspace_written_since(m0), "the probe of the routed trilinear pull left no verdict"
        t.done()


@pytest.mark.parametrize("dtype", TYPES, ids=IDS)
@pytest.mark.parametrize("orders", [[2, 2, 2], [3, 3, 3], [1, 2, 3]], ids=["2", "3", "mixed"])
def test_class_sorted_tiles(orders, dtype, monkeypatch):
    i = sum(orders) + IDS.index(SC.name(dtype))
    C, misalign = _case(i)
    b, ex = MC._bounds(i), i % 3
    vol, src, gvo, grid = MC._problem(360 + i, C, 0.7)
    vol, src, gvo = _stored(dtype, vol, src, gvo)
    ref = _truth(("sorted", tuple(orders), str(dtype)), vol, src, gvo, grid, ISHAPE, b, orders, ex, ("pull", "push", "pullbwd", "pushbwd"))
    t = Tally("class_sorted_tiles")
    with MC.contract(monkeypatch, misalign, "sorted 16-bit") as env:
        _run(env, t, ref, vol, src, gvo, grid, ISHAPE, b, orders, ex, 0, dtype, (orders, b, ex, C, misalign), scatter_flags=MC.SORTED_SCATTER)
    t.done()


@pytest.mark.parametrize("dtype", TYPES, ids=IDS)
@pytest.mark.parametrize("sigma,how", [(0.0, "flag"), (7.0, "backend")])
def test_owner_computes_push(sigma, how, dtype, monkeypatch, routing):
    for order in (3, 2):
        i = order + int(sigma) + IDS.index(SC.name(dtype))
        C, misalign = _case(i)
        b, o, ex = MC._bounds(i), [order] * 3, i % 3
        vol, src, gvo, grid = MC._problem(380 + i, C, sigma)
        src, = _stored(dtype, src)
        ref = _truth(("owner", order, sigma, str(dtype)), vol, src, gvo, grid, ISHAPE, b, o, ex, ("push", "count"))
        backend.rough_deformations = True if how == "backend" else None
        t = Tally("owner_computes_push")
        with MC.contract(monkeypatch, misalign, "owner 16-bit") as env:
            sd, gd = env.put(src, dtype), env.put(grid)
            fl = BINNED if how == "flag" else 0
            what = (order, sigma, how, b, ex, C, misalign)
            t.lp(_hip.scatter("push", sd, gd, list(ISHAPE), b, o, ex, flags=fl), ref["push"], dtype, "push", what)
            both = _hip.scatter("push", sd, gd, list(ISHAPE), b, o, ex, flags=fl, with_count=True)
            t.lp(both[:, :C], ref["push"], dtype, "push+count", what)
            t.lp(both[:, C:], ref["count"], dtype, "push+count: count", what)
            assert env.seam.workspace_was_written()
        t.done()


@pytest.mark.parametrize("dtype", TYPES, ids=IDS)
@pytest.mark.parametrize("sigma,rough", [(0.0, None), (12.0, True)], ids=["lean_tiles", "bricks"])
def test_two_d(sigma, rough, dtype, monkeypatch, routing):
    for k in range(3):
        i = k + int(sigma) + IDS.index(SC.name(dtype))
        o = [1 + i % 3, 1 + (i // 2) % 3]
        b, ex = [i % 7, (i + 3) % 7], (i + o[0]) % 3
        C, misalign = (1, 3, 5)[k], (0, 1, 3)[(k + int(sigma)) % 3]
        vol, src, gvo, grid = MC._problem(400 + i, C, sigma, L2, S2)
        vol, src, gvo = _stored(dtype, vol, src, gvo)
        ref = _truth(("2d", sigma, k, str(dtype)), vol, src, gvo, grid, L2, b, o, ex, ("pull", "push", "count", "pullbwd", "pushbwd"))
        backend.rough_deformations = rough
        t = Tally("bricks_2d" if rough else "lean_tiles_2d")
        with MC.contract(monkeypatch, misalign, "2d 16-bit") as env:
            m0 = env.mark()
            _run(env, t, ref, vol, src, gvo, grid, L2, b, o, ex, 0, dtype, (o, b, ex, C, misalign), with_count=True)
            if rough:
                assert env.workspace_written_since(m0), "no workspace was written: the 2-D bricks did not run"
        t.done()


@pytest.mark.parametrize("dtype", TYPES, ids=IDS)
@pytest.mark.parametrize("flags", [0, NF], ids=["tiles", "generic"])
@pytest.mark.parametrize("order", [1, 3, 7])
def test_push1d(order, flags, dtype, monkeypatch):
    gen = torch.Generator().manual_seed(420 + order)
    for k, (n_in, n_out, zoom, sigma) in enumerate(((5001, 5003, 1.0, 2.0), (4099, 901, 0.22, 3.0))):
        b, ex, C, misalign = [(order + 3 * k) % 7], (order + k) % 3, (1, 3)[(order + k) % 2], (0, 1, 3)[(order + k) % 3]
        src, = _stored(dtype, torch.randn([3, C, n_in], generator=gen))
        grid = (torch.arange(n_in, dtype=torch.float32) * zoom - 2 + sigma * torch.randn([3, n_in], generator=gen))[..., None].contiguous()
        for thr in (-0.55, -0.05, n_out - 1 + 0.05, n_out - 1 + 0.55):
            grid = torch.where((grid - thr).abs() < 1e-3, grid + 4e-3, grid)
        ref = MC._cached(("storage", "1d", order, k, str(dtype)),
                         lambda: (np.asarray(oracle.grid_push(src.double(), grid.double(), [n_out], b, [order], ex)),
                                  np.asarray(oracle.grid_count(grid.double(), [n_out], b, [order], ex))))
        t = Tally("push1d_generic" if flags else "push1d_tiles")
        with MC.contract(monkeypatch, misalign, "push1d 16-bit") as env:
            sd, gd = env.put(src, dtype), env.put(grid)
            what = (order, k, b, ex, C, misalign)
            t.lp(_hip.scatter("push", sd, gd, [n_out], b, [order], ex, flags=flags), ref[0], dtype, "push", what)
            both = _hip.scatter("push", sd, gd, [n_out], b, [order], ex, flags=flags, with_count=True)
            t.lp(both[:, :C], ref[0], dtype, "push+count", what)
            t.lp(both[:, C:], ref[1], dtype, "push+count: count", what)
        t.done()


@pytest.mark.parametrize("dt", IDS)
@pytest.mark.parametrize("name,shape,dim,misalign", [("cols64", (5, 137, 64), 1, 0), ("cols66_off", (5, 137, 66), 1, 3), ("lastdim", (700, 137), 1, 0)])
def test_resample1d_forward(name, shape, dim, misalign, dt):
    """One pass per call (ONE rounding): against the dense float64 pass matrix of tests/separable_truth.py on the stored input."""
    t = Tally("resample1d_" + name)
    i = 0
    for ns in (1100, 53):
        for order in ST.ORDERS:
            kind, (bound, ex) = ST.KINDS[i % 4], ST.rotate(i + len(name))
            i += 1
            lin, W = TS._matrix(kind, ns, shape[dim], dt, bound, order, ex)
            x, x64 = TS._input(shape, dt)
            xd, ld = TS._put(x, misalign), TS._lin(lin, dt)
            got = _hip.resample1d(xd, ld, dim, order, bound, ex, ST.iso_mode(order))
            assert got.shape == shape[:dim] + (ns,) + shape[dim + 1:]
            t.lp(got, ST.apply_forward(x64, W, dim), TS.DT[dt], "forward", (ns, order, kind, bound, ex))
    t.done()


# ---- edges ---------------------------------------------------------------------------------------------------------------------------

def _tie_problem(dtype, lattice, samples, axis, C):
    """A volume whose neighbours along `axis` are ADJACENT numbers of the format (consecutive bit patterns: last bits alternately
    even and odd, the run crosses a power of two, so two binades; sign by the parity of the other indices), and interior samples at
    i + 0.5 along `axis`, at integers along the other dims, all strictly inside the lattice (no bound takes part): the float32 result
    of a linear pull is the exact midpoint."""
    one = int(SC.bits(torch.ones(1, dtype=dtype))[0])
    dim, n = len(lattice), lattice[axis]
    idx = torch.meshgrid(*[torch.arange(m) for m in lattice], indexing="ij")
    other = sum(idx[d] for d in range(dim) if d != axis) if dim > 1 else torch.zeros(lattice, dtype=torch.long)
    vols = []
    for bc in range(2 * C):
        pat = one - n // 2 + 3 * bc + idx[axis] + 5 * (other % 4)              # every run of n patterns contains `one` = 2^0
        pat = pat + 0x8000 * ((other + bc) % 2)                                # sign bit
        vols.append(torch.where(pat >= 0x8000, pat - 0x10000, pat).to(torch.int16).view(dtype))
    vol = torch.stack(vols).reshape(2, C, *lattice)
    coords = [(1 + (torch.arange(m) * (3 if d != axis else 1)) % (lattice[d] - 3)).float() for d, m in enumerate(samples)]   # 1 .. n - 3: interior
    coords[axis] = coords[axis] + 0.5
    grid = torch.stack(torch.meshgrid(*coords, indexing="ij"), -1)[None].expand(2, *samples, dim).contiguous()
    return vol, grid


def _tie_truth(vol, grid, axis):
    """Round-to-nearest-even of the exact midpoint, from float64 (a double converts to the format with one rounding)."""
    dim = grid.shape[-1]
    g = grid[0].long()                                                          # (floor: i along `axis`, the integer elsewhere)
    lo = [g[..., d] for d in range(dim)]
    hi = [g[..., d] + (1 if d == axis else 0) for d in range(dim)]
    v = vol.double()
    a = v[(slice(None), slice(None)) + tuple(lo)]
    mid = 0.5 * (a + v[(slice(None), slice(None)) + tuple(hi)])
    assert torch.equal(mid.float().double(), mid)                               # exact in float32
    want = mid.to(vol.dtype)
    return want, float((want.double() == a).double().mean())                    # (and how often the tie goes to the sample's left neighbour)


TIE_ROUTES = {1: [("generic", NF, None), ("default", 0, None)],
              2: [("generic", NF, None), ("lean_tiles", 0, None), ("bricks", 0, True), ("lds_tiles", TILED, None)],
              3: [("generic", NF, None), ("lds_tiles", TILED, None), ("sorted_tiles", BINNED, None), ("routed", 0, None)]}


@pytest.mark.parametrize("dtype", TYPES, ids=IDS)
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_ties_round_to_even_bit_for_bit(dim, dtype, pinned_handback, routing):
    pinned_handback("never")
    lattice, samples = {1: ((901,), (4099,)), 2: (L2, S2), 3: (ISHAPE, OSHAPE)}[dim]
    bad = []
    for axis in range(dim):
        for C in (1, 3):
            vol, grid = _tie_problem(dtype, lattice, samples, axis, C)
            want, left = _tie_truth(vol, grid, axis)
            assert 0.25 < left < 0.75                                           # both directions are asked for: up and down, in magnitude too
            assert float(want.float().abs().min()) < 1.0 < float(want.float().abs().max()) and bool((want < 0).any()) and bool((want > 0).any())
            vd, gd = vol.to(DEV), grid.to(DEV)
            for name, fl, rough in TIE_ROUTES[dim]:
                backend.rough_deformations = rough
                got = _hip.gather("pull", vd, gd, [(axis + 2 * d) % 7 for d in range(dim)], [1] * dim, 1, flags=fl)
                assert got.dtype == dtype
                miss = SC.mismatch(got, want)
                print("STORAGE ties_%dd_%s bits_that_differ %s %.4f %.4f" % (dim, name, SC.name(dtype), miss, SC.ulps(got.double().cpu().numpy(), want.double().numpy(), dtype)))
                if miss:
                    bad.append((name, axis, C, miss))
    assert not bad, "ties not rounded to even (route, axis, C, fraction of the outputs): %s" % bad


@pytest.mark.parametrize("dtype", TYPES, ids=IDS)
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_order_zero_pull_is_an_exact_gather(dim, dtype, pinned_handback):
    """Nearest neighbour: every output is a stored value, its negative (the antisymmetric bounds) or zero -- no arithmetic to round.
    (Coordinates within 1e-3 of a half integer are moved off it: there float32 and float64 pick different neighbours.)"""
    pinned_handback("never")
    lattice, samples = {1: ((901,), (4099,)), 2: (L2, S2), 3: (ISHAPE, OSHAPE)}[dim]
    for k, (fl, C) in enumerate(((NF, 3), (0, 1), (TILED, 3))):
        i = dim + k
        b, ex = MC._bounds(i, dim), i % 3
        vol, src, gvo, grid = MC._problem(440 + i, C, 2.0, lattice, samples)
        vol, = _stored(dtype, vol)
        frac = grid - torch.floor(grid)
        grid = torch.where((frac - 0.5).abs() < 1e-3, grid + 4e-3, grid)
        want = MC._cached(("storage", "nearest", dim, k, str(dtype)), lambda: np.asarray(oracle.grid_pull(vol.double().numpy(), grid.double().numpy(), b, [0] * dim, ex)))
        got = _hip.gather("pull", vol.to(dtype).to(DEV), grid.to(DEV), b, [0] * dim, ex, flags=fl)
        assert got.dtype == dtype
        g = got.double().cpu().numpy()
        assert np.array_equal(g, want), ("order 0", dim, fl, b, ex, int((g != want).sum()), g.size)


def _bump_problem(dtype, order):
    """A smooth bump on a zero background, bound 'zero': the pulled values fall from max|want| through six decades to exact zeros."""
    n = torch.tensor(ISHAPE, dtype=torch.float64)
    c, s = (n - 1) / 2, torch.tensor([6.5, 5.2, 8.0], dtype=torch.float64)
    idx = torch.stack(torch.meshgrid(*[torch.arange(m, dtype=torch.float64) for m in ISHAPE], indexing="ij"), -1)
    bump = torch.exp(-0.5 * (((idx - c) / s) ** 2).sum(-1))
    vol = torch.stack([bump, -0.75 * bump, 0.5 * bump]).reshape(1, 3, *ISHAPE).expand(2, 3, *ISHAPE)
    vol, = _stored(dtype, vol.float())
    gen = torch.Generator().manual_seed(460 + order)
    lin = []
    for d, m in enumerate(OSHAPE):                         # samples denser near the middle, reaching past the lattice's ends
        u = torch.linspace(-1, 1, m)
        lin.append(float(c[d]) + (float(c[d]) + 1.5) * u.sign() * u.abs() ** 1.5)
    grid = torch.stack(torch.meshgrid(*lin, indexing="ij"), -1)[None] + 0.3 * torch.randn([2, *OSHAPE, 3], generator=gen)
    return vol.contiguous(), grid.float().contiguous()


@pytest.mark.parametrize("dtype", TYPES, ids=IDS)
@pytest.mark.parametrize("order", [1, 3])
def test_small_outputs_are_held_to_their_own_half_ulp(order, dtype, pinned_handback):
    pinned_handback("never")
    vol, grid = _bump_problem(dtype, order)
    b, o, ex = [0] * 3, [order] * 3, 1                      # bound 'zero' (include/interpol_hip.h: code 0)
    want = MC._cached(("storage", "bump", order, str(dtype)), lambda: np.asarray(oracle.grid_pull(vol.double().numpy(), grid.double().numpy(), b, o, ex)))
    a = np.abs(want)
    scale = float(a.max())
    assert a[a > 0].min() < 1e-6 * scale and (a == 0).any(), "the truth does not span six decades and the background"
    by_ulp = float((0.5 * SC.ulp16(want, dtype) > 1e-5 * scale).mean())
    print("small outputs %s order %d: %.1f %% of the elements judged by their half ulp" % (SC.name(dtype), order, 100 * by_ulp))
    assert by_ulp >= 0.25
    t = Tally("small_outputs")
    for name, fl in (("generic", NF), ("lds_tiles", TILED), ("default", 0)):
        got = _hip.gather("pull", vol.to(dtype).to(DEV), grid.to(DEV), b, o, ex, flags=fl)
        t.lp(got, want, dtype, "pull " + name, (order,))
    t.done()


@pytest.mark.parametrize("order", [1, 3])
def test_f16_subnormal_results(order, pinned_handback):
    """Data scaled by 2^-17: stored values and truth in f16's subnormal range 2^-24 .. 2^-14, where the spacing is 2^-24 throughout."""
    pinned_handback("never")
    dtype = torch.float16
    b, o, ex = MC._bounds(order), [order] * 3, 1
    vol, src, gvo, grid = MC._problem(480 + order, 3, 1.0)
    vol, src = _stored(dtype, vol * 2.0 ** -17, src * 2.0 ** -17)
    ref = _truth(("subnormal", order), vol, src, gvo, grid, ISHAPE, b, o, ex, ("pull", "push"))
    for k in ("pull", "push"):
        a = np.abs(ref[k])
        assert float((a < 2.0 ** -14).mean()) > 0.9 and float(((a >= 2.0 ** -24) & (a < 2.0 ** -14)).mean()) > 0.5, k
    t = Tally("f16_subnormal")
    vd, sd, gd = vol.to(dtype).to(DEV), src.to(dtype).to(DEV), grid.to(DEV)
    for name, fl in (("generic", NF), ("lds_tiles", TILED), ("owner", BINNED)):
        if fl != BINNED:
            t.lp(_hip.gather("pull", vd, gd, b, o, ex, flags=fl), ref["pull"], dtype, "pull " + name, (order,))
        t.lp(_hip.scatter("push", sd, gd, list(ISHAPE), b, o, ex, flags=fl), ref["push"], dtype, "push " + name, (order,))
    t.done()


def _check_overflow(t, got, want, op):
    want = np.asarray(want, dtype=np.float64)
    e = SC.e32(want, np.abs(want).max())
    a = np.abs(want)
    over, under = a > SC.F16_INF_FROM + e, a < SC.F16_INF_FROM - e
    assert bool((over | under).all()), "an element of the truth lies in the band around 65520: the case decides nothing there"
    assert int(over.sum()) >= 10 and int(under.sum()) >= 10, "the case has gone empty"
    g = got.detach().double().cpu().numpy()
    assert np.array_equal(np.isinf(g), over) and np.array_equal(np.sign(g[over]), np.sign(want[over])), (op, "inf exactly where the truth is past 65520")
    t.lp(got.reshape(-1)[torch.from_numpy(under.reshape(-1))], want[under], torch.float16, op)


def test_f16_overflow_of_a_push(pinned_handback):
    """Sums past 65504: inf exactly where the truth exceeds 65520 + e32 (65504 plus half a spacing of 32), finite and within the bar below
    65520 - e32; the field leaves no element of the truth inside that band (asserted)."""
    pinned_handback("never")
    dtype = torch.float16
    gen = torch.Generator().manual_seed(500)
    t = Tally("f16_overflow")
    # 1-D, 4099 -> 901: some 4.5 samples per lattice point, item 0 positive, item 1 negative
    n_in, n_out = 4099, 901
    src = 4000.0 + 26000.0 * torch.rand([2, 1, n_in], generator=gen)
    src[1] = -src[1]
    src, = _stored(dtype, src)
    grid = (torch.arange(n_in, dtype=torch.float32) * 0.22 - 2 + 1.0 * torch.randn([2, n_in], generator=gen))[..., None].contiguous()
    want = np.asarray(oracle.grid_push(src.double(), grid.double(), [n_out], [1], [3], 1))
    for name, fl in (("push1d_tiles", 0), ("push1d_generic", NF)):
        _check_overflow(t, _hip.scatter("push", src.to(dtype).to(DEV), grid.to(DEV), [n_out], [1], [3], 1, flags=fl), want, "push " + name)
    # 3-D, (37, 45, 29) samples onto (19, 17, 25): some 6 per lattice point
    lattice = (19, 17, 25)
    _, src, _, grid = MC._problem(501, 1, 1.0, lattice, OSHAPE)
    src = 2000.0 + 22000.0 * torch.rand(src.shape, generator=gen)
    src[1] = -src[1]
    src, = _stored(dtype, src)
    want = MC._cached(("storage", "overflow3d"), lambda: np.asarray(oracle.grid_push(src.double().numpy(), grid.double().numpy(), list(lattice), [1, 4, 6], [3] * 3, 1)))
    for name, fl in (("lds_tiles", TILED), ("owner", BINNED), ("generic", NF)):
        _check_overflow(t, _hip.scatter("push", src.to(dtype).to(DEV), grid.to(DEV), list(lattice), [1, 4, 6], [3] * 3, 1, flags=fl), want, "push " + name)
    t.done()
