"""Owner-computes push (csrc/push_owner.hip): the first-writer flush of the colour launches against load + add + store everywhere
(INTERPOL_FLAG_RMW_FLUSH) on the same inputs.

A colour launch stores, without a load, the points of a brick's box that no earlier colour's box holds (csrc/owner_geom.hpp:
fresh_range): the load would return the zero of the call's own zero-fill, and 0.f + x == x for every x the flush decodes.  So wherever
the push is bit-reproducible (dct2 / replicate / dct1, every stencil within 9 points of the lattice: see tests/test_lean_kernels.py)
the two sides must agree bit for bit: torch.equal.  The hazard is what own_bin adds to the zero-filled target BEFORE colour 0 with
float atomics (scatter_orphans: thin shell runs; scatter_direct: far samples): own_bin marks the bricks it wrote under, and those keep
load + add + store -- test_direct_scatters_are_kept fails if a store eats such a sample.

Shapes.  (96, 80, 104) is the lattice of tests/test_lean_kernels.py.  (84, 83, 100): n = 84 gives the folding dims a short brick of
exactly K = 3 cells at `split` (the largest overlap the grid allows: the fresh range of an odd neighbour is empty on that side), n = 83
makes brick_grid drop the short brick -- test_brick_grid_of_the_second_shape redoes brick_grid's arithmetic.  Dropping it takes the
brick's 2 cells off the interior: its first taps end at n + 3, not n + 5, so at n = 83 a displacement clamped to +-6 DOES reach a shell
brick (sample 82 at 82 + 6 = 88: first tap 87 = top), own_bin scatters those strays with float atomics and the push is no longer
reproducible against itself there.  The bit-equality cases of that shape therefore clamp to +-4 (first taps <= n + 2: no shell, no
direct scatter, as the recipe intends); the +-6 field on it is kept as a case of its own at the bar for float atomics."""
import numpy as np
import pytest
import torch

import golden_util as G
import interpol
from oracle import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPLICATE, DCT1, DCT2 = 1, 2, 3
SHAPES = {"lean": (96, 80, 104), "short": (84, 83, 100)}
AMP = {"lean": 6.0, "short": 4.0}            # clamp of the displacement that keeps every first tap in an interior brick (module docstring)


def test_bound_codes():
    from interpol.codes import bound_to_code
    assert [bound_to_code(b) for b in ("replicate", "dct1", "dct2")] == [REPLICATE, DCT1, DCT2]


def _brick_dim(n, K, BR=16, BOX=19):
    """brick_grid_dim of a folding dim (csrc/owner_geom.hpp): cells, bricks, cells of the short brick (0: none)."""
    lo, top = -(BOX - 1) // 2, n - (BOX + 1) // 2 + BR
    nin = (top - lo + BR - 1) // BR
    c = top - lo - BR * (nin - 1)
    if c < K:
        top -= c
        nin -= 1
        c = BR
    return top - lo, nin, (c if c < BR else 0)


def test_brick_grid_of_the_second_shape():
    assert _brick_dim(84, 3) == (99, 7, 3)            # a short brick of exactly K = 3 cells
    assert _brick_dim(83, 3) == (96, 6, 0)            # c = 2 < K: dropped, six whole bricks
    assert _brick_dim(100, 3)[2] == 3 and _brick_dim(96, 3)[2] == 15 and _brick_dim(80, 3)[2] == 15 and _brick_dim(104, 3)[2] == 7


_INPUTS = {}


def _inputs(B, C, seed, shape=SHAPES["lean"], amp=6.0, sigma=2.0):
    """The recipe of test_lean_kernels._inputs on `shape`: identity + i.i.d. noise of `sigma` voxels clamped to +-amp (amp <= 6: every
    stencil of a cubic stays within 9 points of the lattice -- no shell, no direct scatter).  Built once per key."""
    key = (B, C, seed, tuple(shape), amp, sigma)
    if key not in _INPUTS:
        g = torch.Generator().manual_seed(seed)
        src = torch.randn([B, C, *shape], generator=g)
        disp = (sigma * torch.randn([B, *shape, 3], generator=g)).clamp(-amp, amp)
        grid = (interpol.identity_grid(shape)[None] + disp).contiguous()
        _INPUTS[key] = (src.to(DEV), grid.to(DEV), list(shape))
    return _INPUTS[key]


def _push(src, grid, shape, bound, order, rmw, flags=None, **kw):
    from interpol import _hip
    fl = _hip.FLAG_BINNED_SCATTER if flags is None else flags
    if rmw:
        fl |= _hip.FLAG_RMW_FLUSH
    return _hip.scatter("push", src, grid, shape, [bound] * 3, [order] * 3, 1, flags=fl, **kw)


def test_flag_value_and_api_never_sets_it(monkeypatch):
    """Bit 29, outside the other flags and the debug bits (8 - 23); the Python API (grid_push, grid_count and the backward of
    grid_pull, which pushes) never hands it to _hip.scatter."""
    from interpol import _hip
    assert _hip.FLAG_RMW_FLUSH == 1 << 29
    assert not _hip.FLAG_RMW_FLUSH & (_hip.FLAG_SHELL_RUNS | _hip.FLAG_GENERAL_KERNELS | _hip.FLAG_SERIAL_ITEMS | _hip.FLAG_AUTO_SCATTER
                                      | _hip.FLAG_SMALL_TILES | 0xffffff)
    seen = []
    real = _hip.scatter

    def spy(*a, **kw):
        seen.append(int(kw.get("flags", a[7] if len(a) > 7 else 0)))
        return real(*a, **kw)
    monkeypatch.setattr(_hip, "scatter", spy)
    src, grid, shape = _inputs(2, 2, 50, shape=(48, 48, 48))
    src = src.clone().requires_grad_(True)
    interpol.grid_push(src, grid, shape, interpolation=3, bound="dct2", extrapolate=True).sum().backward()
    interpol.grid_count(grid, shape, interpolation=3, bound="dct2", extrapolate=True)
    x = src.detach().clone().requires_grad_(True)
    interpol.grid_pull(x, grid, interpolation=3, bound="dct2", extrapolate=True).sum().backward()
    assert len(seen) >= 2, seen
    assert not any(f & _hip.FLAG_RMW_FLUSH for f in seen), seen


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C", [1, 2, 3])
@pytest.mark.parametrize("bound", [DCT2, REPLICATE, DCT1])
@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("shape", ["lean", "short"])
def test_first_writer_equals_rmw(shape, order, bound, C, B):
    """One chain (B = 1) and two (B = 3); the odd channel counts end on a pair with one channel."""
    src, grid, shp = _inputs(B, C, 100 + 10 * B + C, shape=SHAPES[shape], amp=AMP[shape])
    a = _push(src, grid, shp, bound, order, rmw=False)
    b = _push(src, grid, shp, bound, order, rmw=True)
    assert float(b.abs().max()) > 0
    if not torch.equal(a, b):
        print("max |first writer - rmw| = %.3e, max |rmw| = %.3e" % (float((a - b).abs().max()), float(b.abs().max())))
    assert torch.equal(a, b), (shape, order, bound, C, B)


@pytest.mark.parametrize("bound", [DCT2, REPLICATE, DCT1])
def test_strays_of_the_dropped_short_brick(bound):
    """(84, 83, 100) with the clamp at +-6: at n = 83 the samples clamped to +6 on the high face have their first tap in a shell brick,
    a few per sample tile -- own_bin scatters them itself in front of colour 0 (float atomics: several of them on one point under
    replicate) and marks the bricks under them.  Both sides within the bar of a different order of float additions, 1e-6 max|ref|."""
    src, grid, shp = _inputs(3, 2, 132, shape=SHAPES["short"], amp=6.0)
    assert float(grid[..., 1].max()) == SHAPES["short"][1] - 1 + 6.0      # (a stray exists: first tap 87 = top of dim 1)
    a = _push(src, grid, shp, bound, 3, rmw=False)
    b = _push(src, grid, shp, bound, 3, rmw=True)
    dev, scale = float((a - b).abs().max()), float(b.abs().max())
    print("max |first writer - rmw| = %.3e = %.3e of max |rmw|" % (dev, dev / scale))
    assert dev <= 1e-6 * scale, (dev, scale)


# ---- own_bin's direct scatters
MOVES = (  # (sample, {dim: voxels outside the lattice; < 0: below index 0, > 0: above index n - 1})
    ((5, 5, 5), {0: -40.3}),
    ((20, 40, 60), {1: 45.6}),
    ((50, 30, 90), {2: -300.4}),
    ((70, 70, 10), {0: 299.7}),
    ((90, 10, 50), {0: -60.2, 2: 100.6}),
    ((40, 60, 40), {1: -150.1}),
    ((41, 61, 41), {1: -220.8, 2: 41.5}),          # the same sample tile as the one above
)
_DIRECT = {}


def _direct_case():
    """The rough field of _inputs with a handful of samples (at most two per sample tile) moved 40 to 300 voxels outside the lattice:
    first taps inside [-160, n + 160) are binned into shell bricks, and a tile's few make a thin run -- scatter_orphans; beyond, and
    for the other samples of a tile that a stray spreads over more than six bricks -- scatter_direct.  `bare`: the same sources with
    the moved samples' values zeroed (they add nothing).  Oracles: float64, once."""
    if not _DIRECT:
        B, C = 2, 2
        src, grid, shape = _inputs(B, C, 900)
        src, grid = src.cpu().clone(), grid.cpu().clone()
        bare = src.clone()
        for b in range(B):
            for at, out in MOVES:
                for d, v in out.items():
                    grid[(b, *at, d)] = v if v < 0 else shape[d] - 1 + v
                assert float(src[(b, 0, *at)]) != 0.0
                bare[(b, slice(None), *at)] = 0.0
        oracle.set_threads(8)
        try:
            want = np.asarray(oracle.grid_push(src.double(), grid.double(), shape, [DCT2], [3], 1))
            want_bare = np.asarray(oracle.grid_push(bare.double(), grid.double(), shape, [DCT2], [3], 1))
        finally:
            oracle.set_threads(1)
        _DIRECT.update(src=src.to(DEV), bare=bare.to(DEV), grid=grid.to(DEV), shape=shape, want=want, want_bare=want_bare)
    return _DIRECT


def test_direct_scatters_are_kept():
    c = _direct_case()
    shape, want = c["shape"], c["want"]
    scale = float(np.abs(want).max())
    fw = _push(c["src"], c["grid"], shape, DCT2, 3, rmw=False)
    rmw = _push(c["src"], c["grid"], shape, DCT2, 3, rmw=True)
    # the owner tests' bar against the float64 oracle, both sides
    G.assert_close(fw.cpu().numpy(), want, 1e-5, 1e-5, "first-writer push with direct scatters")
    G.assert_close(rmw.cpu().numpy(), want, 1e-5, 1e-5, "rmw push with direct scatters")
    # the two sides: float atomics land in another order, nothing else differs
    dev = float((fw - rmw).abs().max())
    print("first writer against rmw: max |difference| %.3e = %.3e of max |ref|" % (dev, dev / scale))
    assert dev <= 1e-6 * scale, (dev, scale)
    # a store that ate a moved sample would make the result that of the sources WITHOUT the moved samples at the points under its
    # stencil: there the two results must differ, by what the oracle says the moved samples add
    fw_bare = _push(c["bare"], c["grid"], shape, DCT2, 3, rmw=False)
    G.assert_close(fw_bare.cpu().numpy(), c["want_bare"], 1e-5, 1e-5, "first-writer push without the moved samples")
    added = want - c["want_bare"]
    under = np.abs(added) > 1e-3 * scale                                # points where the moved samples weigh in clearly
    assert int(under.sum()) >= 64, int(under.sum())
    got = (fw - fw_bare).cpu().numpy().astype(np.float64)
    assert np.all(got[under] != 0.0)
    err = float(np.abs(got - added)[under].max())
    print("moved samples: %d points under their stencils, max |added - oracle| %.3e (bar %.3e)" % (int(under.sum()), err, 2e-5 * scale))
    assert err <= 2e-5 * scale, (err, scale)                            # (the difference of two results that each meet 1e-5 max|ref|)


def test_accumulate_adds_into_the_preload():
    """INTERPOL_FLAG_ACCUMULATE: the library does not zero-fill, no first-writer store -- the result is preload + push on both sides."""
    from interpol import _hip
    src, grid, shape = _inputs(3, 2, 700)
    base = torch.randn([3, 2, *shape], generator=torch.Generator().manual_seed(5)).to(DEV)
    a, b = base.clone(), base.clone()
    _push(src, grid, shape, DCT2, 3, rmw=False, flags=_hip.FLAG_BINNED_SCATTER | _hip.FLAG_ACCUMULATE, out=a)
    _push(src, grid, shape, DCT2, 3, rmw=True, flags=_hip.FLAG_BINNED_SCATTER | _hip.FLAG_ACCUMULATE, out=b)
    assert torch.equal(a, b)
    push = _push(src, grid, shape, DCT2, 3, rmw=True)
    # preload + push: the colours add up to eight boxes per point ONTO the preload, so the roundings differ from base + (sum of boxes)
    tol = 1e-5 * float((base.abs() + push.abs()).max())
    assert float((a - (base + push)).abs().max()) <= tol
    assert float((a - base).abs().max()) > 0.5 * float(push.abs().max())


def test_user_target_full_of_nan_is_zero_filled():
    """out= without the accumulate flag: the library's zero-fill still runs, no NaN of the caller's survives a first-writer store or a
    load + add + store; equal to a fresh target bit for bit."""
    src, grid, shape = _inputs(3, 2, 710)
    out = torch.full([3, 2, *shape], float("nan"), device=DEV)
    _push(src, grid, shape, DCT2, 3, rmw=False, out=out)
    assert not bool(torch.isnan(out).any())
    assert torch.equal(out, _push(src, grid, shape, DCT2, 3, rmw=True))


def test_shared_target_equals_rmw(monkeypatch):
    """3 sources of 48^3 into ONE 96^3 target (interpol.distributed.push_count_shared: batch stride 0, the items share the bricks, the
    caller zero-filled the target and the call accumulates): no first-writer store -- equal to the rmw side bit for bit."""
    from interpol import _hip
    from interpol.distributed import push_count_shared
    g = torch.Generator().manual_seed(800)
    n, N = 48, 96
    src = torch.randn([3, 2, n, n, n], generator=g)
    grid = (interpol.identity_grid([n] * 3)[None] * (N / n) + 2.0 * torch.randn([3, n, n, n, 3], generator=g).clamp(-3.0, 3.0)).contiguous()
    src, grid = src.to(DEV), grid.to(DEV)
    real, seen = _hip.scatter, []

    def run(extra):
        def with_flag(*a, **kw):
            # (the owner-computes organisation on both sides: _hip.scatter adds its probe routing only to calls without high flag bits)
            kw["flags"] = int(kw.get("flags", 0)) | _hip.FLAG_BINNED_SCATTER | extra
            seen.append((kw["flags"], bool(kw.get("shared", False))))
            return real(*a, **kw)
        monkeypatch.setattr(_hip, "scatter", with_flag)
        try:
            return push_count_shared(src, grid, [N] * 3, interpolation=3, bound="dct2", extrapolate=True, reduce="none")
        finally:
            monkeypatch.setattr(_hip, "scatter", real)
    pa, ca = run(0)
    pb, cb = run(_hip.FLAG_RMW_FLUSH)
    assert seen and all(s for _, s in seen), seen                       # (the shared target went through _hip.scatter)
    assert any(f & _hip.FLAG_RMW_FLUSH for f, _ in seen) and all(f & _hip.FLAG_ACCUMULATE for f, _ in seen)
    assert float(pb.abs().max()) > 0 and float(cb.max()) > 0
    assert torch.equal(pa, pb) and torch.equal(ca, cb)
