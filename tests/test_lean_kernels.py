"""Owner-computes push (csrc/push_owner.hip): the colour instantiation of own_accumulate (SHELL = false: the default for the
colour launches of orders 1 / 2 / 3) against the general kernel for every launch (INTERPOL_FLAG_GENERAL_KERNELS) on the same inputs.

The colour instantiation drops paths and unswitches modes; it adds the same numbers.  Inside a brick the sums are integers, and the
up to eight boxes that meet at a lattice point are added in the fixed order of the colours.  So wherever the general kernel is
bit-reproducible (dct2 / replicate / dct1, every stencil within 9 points of the lattice: no shell launch, no direct scatter) the
two must agree bit for bit: torch.equal.  That holds for the 64-bit sums of a dense brick too.  Where float atomics take part
neither kernel is reproducible against itself:
  * the shell launch (dft, zero): both sides against the float64 oracle at the bar of the owner tests (rtol 1e-5 + 1e-5 max|ref|);
  * a brick with a non-finite source adds ALL its records with float atomics, in no order: see _nonfinite_inputs."""
import numpy as np
import pytest
import torch

import golden_util as G
import interpol
from oracle import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPLICATE, DCT1, DCT2, DFT, ZERO = 1, 2, 3, 6, 0


def test_bound_codes():
    from interpol.codes import bound_to_code
    assert [bound_to_code(b) for b in ("replicate", "dct1", "dct2", "dft", "zero")] == [REPLICATE, DCT1, DCT2, DFT, ZERO]


def _inputs(B, C, seed, amp=6.0, sigma=2.0, n=96):
    """Sources and a dense grid on (96, 80, 104) -- interior bricks and bricks at the folding ends of every dim: identity + i.i.d.
    noise of `sigma` voxels, clamped to +-amp (amp <= 6: every stencil of a cubic stays within 9 points of the lattice -- nothing
    reaches the shell bricks or the direct scatter)."""
    g = torch.Generator().manual_seed(seed)
    shape = (n, n - 16, n + 8)
    src = torch.randn([B, C, *shape], generator=g)
    disp = sigma * torch.randn([B, *shape, 3], generator=g)
    if amp is not None:
        disp = disp.clamp(-amp, amp)
    grid = (interpol.identity_grid(shape)[None] + disp).contiguous()
    return src.to(DEV), grid.to(DEV), list(shape)


def _push(src, grid, shape, bound, order, general, flags=None, **kw):
    from interpol import _hip
    fl = _hip.FLAG_BINNED_SCATTER if flags is None else flags
    if general:
        fl |= _hip.FLAG_GENERAL_KERNELS
    order = order if isinstance(order, (list, tuple)) else [order] * 3
    return _hip.scatter("push", src, grid, shape, [bound] * 3, list(order), 1, flags=fl, **kw)


def test_flag_value_and_api_never_sets_it(monkeypatch):
    """Bit 27, outside the other flags and the debug bits (8 - 23); the Python API (grid_push, grid_count and the backward of
    grid_pull, which pushes) never hands it to _hip.scatter."""
    from interpol import _hip
    assert _hip.FLAG_GENERAL_KERNELS == 1 << 27
    assert not _hip.FLAG_GENERAL_KERNELS & (_hip.FLAG_SERIAL_ITEMS | _hip.FLAG_AUTO_SCATTER | _hip.FLAG_SMALL_TILES | 0xffff00)
    seen = []
    real = _hip.scatter

    def spy(*a, **kw):
        seen.append(int(kw.get("flags", a[7] if len(a) > 7 else 0)))
        return real(*a, **kw)
    monkeypatch.setattr(_hip, "scatter", spy)
    src, grid, shape = _inputs(2, 2, 50, n=48)
    src.requires_grad_(True)
    interpol.grid_push(src, grid, shape, interpolation=3, bound="dct2", extrapolate=True).sum().backward()
    interpol.grid_count(grid, shape, interpolation=3, bound="dct2", extrapolate=True)
    x = src.detach().clone().requires_grad_(True)
    interpol.grid_pull(x, grid, interpolation=3, bound="dct2", extrapolate=True).sum().backward()
    assert len(seen) >= 2, seen
    assert not any(f & _hip.FLAG_GENERAL_KERNELS for f in seen), seen


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C", [1, 2, 3])
@pytest.mark.parametrize("with_count", [False, True])
def test_lean_equals_general_batch_channels_count(B, C, with_count):
    src, grid, shape = _inputs(B, C, 100 + 10 * B + C)
    a = _push(src, grid, shape, DCT2, 3, general=False, with_count=with_count)
    b = _push(src, grid, shape, DCT2, 3, general=True, with_count=with_count)
    assert a.shape[1] == C + int(with_count) and float(b.abs().max()) > 0
    assert torch.equal(a, b), (B, C, with_count)


@pytest.mark.parametrize("order", [1, 2, 3, (1, 3, 2)])
@pytest.mark.parametrize("bound", [DCT2, REPLICATE, DCT1])
def test_lean_equals_general_orders_and_bounds(order, bound):
    """(1, 3, 2): mixed orders keep ONE instantiation (KMIX, the general kernel, with or without the flag) -- that case only pins
    that the flag disturbs nothing there."""
    src, grid, shape = _inputs(3, 2, 300)
    a = _push(src, grid, shape, bound, order, general=False)
    b = _push(src, grid, shape, bound, order, general=True)
    assert float(b.abs().max()) > 0
    assert torch.equal(a, b), (order, bound)


@pytest.mark.parametrize("order", [1, 2, 3])
def test_dense_brick_takes_the_wide_sums(order):
    """48^3 sources contracted into a 6^3 region of a 48^3 target: 512 samples per lattice point, far beyond what 32-bit channel
    pairs hold -- the brick sums 64 bits per slot, one channel per pass (the colour instantiation: a tap loop of its own)."""
    n = 48
    g = torch.Generator().manual_seed(410 + order)
    src = torch.randn([2, 2, n, n, n], generator=g)
    ident = interpol.identity_grid([n] * 3)[None]
    grid = (21.3 + ident * (6.0 / n) + 0.01 * torch.randn([2, n, n, n, 3], generator=g)).contiguous()
    src, grid = src.to(DEV), grid.to(DEV)
    a = _push(src, grid, [n] * 3, DCT2, order, general=False, with_count=True)
    b = _push(src, grid, [n] * 3, DCT2, order, general=True, with_count=True)
    assert float(b[:, 2].max()) > 100.0                                # (the count channel: hundreds of samples per point)
    assert torch.equal(a, b), order


def _nonfinite_inputs(seed):
    """One inf source in an interior brick (item 0), one nan source on a corner of the sample grid (item 1: its sub-lattice holds
    the faces x = 0, y = 79 and z = 103, whose stencils leave the lattice and wrap at every order); item 2 is the usual rough field.  own_bin folds a sample TILE's max |source| into every brick the tile reaches, so all those bricks leave the fixed
    point and add ALL their records to the target with float atomics, in no order -- reproducible only where a lattice point
    receives at most one non-zero addend that way.  So the two items are sparse: sources zero except on a sub-lattice of stride 12,
    and a third of the displacement everywhere (|d| <= 2: the kept samples lie 8 points apart and more, no two cubic stencils meet)."""
    src, grid, shape = _inputs(3, 2, seed)
    ident = interpol.identity_grid(shape).to(DEV)
    for b, c, at, value in ((0, 0, (40, 37, 51), float("inf")), (1, 1, (0, 79, 103), float("nan"))):
        sub = tuple(slice(a % 12, None, 12) for a in at)
        keep = src[b][(slice(None),) + sub].clone()
        src[b].zero_()
        src[b][(slice(None),) + sub] = keep
        grid[b] = ident + 0.3 * (grid[b] - ident)
        assert float(src[b, c][at]) != 0.0                              # (on the sub-lattice)
        src[b, c][at] = value
    return src, grid, shape


@pytest.mark.parametrize("order", [1, 2, 3])
def test_nonfinite_sources(order):
    """The colour instantiation sends the records of such a brick through float_records, the general kernel through
    scatter_one_thread inside its tap loop: equal finite values, equal NaN masks (the bits of a NaN are nobody's contract)."""
    src, grid, shape = _nonfinite_inputs(500 + order)
    a = _push(src, grid, shape, DCT2, order, general=False)
    b = _push(src, grid, shape, DCT2, order, general=True)
    na, nb = torch.isnan(a), torch.isnan(b)
    assert bool(na.any()) and bool(torch.isinf(a).any())
    assert torch.equal(na, nb)
    assert torch.equal(a[~na], b[~nb]), order


_ORACLE = {}


def _oracle_push(key, src, grid, shape, bound, order):
    """float64 reference, computed once per case and shared by the two sides."""
    if key not in _ORACLE:
        oracle.set_threads(8)
        try:
            _ORACLE[key] = np.asarray(oracle.grid_push(src.cpu().double(), grid.cpu().double(), shape, [bound], [order], 1))
        finally:
            oracle.set_threads(1)
    return _ORACLE[key]


@pytest.mark.parametrize("bound", [DFT, ZERO])
@pytest.mark.parametrize("general", [False, True])
def test_shell_against_the_oracle(bound, general):
    """dft and zero with sigma = 6: the stencils that leave the lattice go to the shell launch (the general kernel on both sides,
    global float atomics) next to the colour launches.  Both sides against the float64 oracle."""
    src, grid, shape = _inputs(2, 2, 600 + bound, amp=None, sigma=6.0)
    got = _push(src, grid, shape, bound, 3, general=general)
    want = _oracle_push(("shell", bound), src, grid, shape, bound, 3)
    G.assert_close(got.cpu().numpy(), want, 1e-5, 1e-5, ("shell push", bound, general))


def test_accumulate_equals_general():
    """INTERPOL_FLAG_ACCUMULATE: no zero-fill, the bricks add into what the target holds."""
    from interpol import _hip
    src, grid, shape = _inputs(3, 2, 700)
    base = torch.randn([3, 2, *shape], generator=torch.Generator().manual_seed(5)).to(DEV)
    a, b = base.clone(), base.clone()
    _push(src, grid, shape, DCT2, 3, general=False, flags=_hip.FLAG_BINNED_SCATTER | _hip.FLAG_ACCUMULATE, out=a)
    _push(src, grid, shape, DCT2, 3, general=True, flags=_hip.FLAG_BINNED_SCATTER | _hip.FLAG_ACCUMULATE, out=b)
    assert not torch.equal(a, base)
    assert torch.equal(a, b)


def test_default_routing_serial_items_and_shared_target():
    """The probe-routed default, the single-stream schedule and a target shared by the items (colour launches with plain stores
    there too) run the colour instantiation as well."""
    from interpol import _hip
    src, grid, shape = _inputs(3, 2, 710)
    want = _push(src, grid, shape, DCT2, 3, general=True)
    assert torch.equal(_push(src, grid, shape, DCT2, 3, general=False, flags=_hip.FLAG_AUTO_SCATTER), want)
    assert torch.equal(_push(src, grid, shape, DCT2, 3, general=False, flags=_hip.FLAG_BINNED_SCATTER | _hip.FLAG_SERIAL_ITEMS), want)
    a = _push(src, grid, shape, DCT2, 3, general=False, shared=True)
    b = _push(src, grid, shape, DCT2, 3, general=True, shared=True)
    assert a.shape[0] == 1 and torch.equal(a, b)


def test_side_stream_of_the_caller_equals_general():
    src, grid, shape = _inputs(3, 2, 720)
    want = _push(src, grid, shape, DCT2, 3, general=True)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        got = _push(src, grid, shape, DCT2, 3, general=False)
        twice = got * 2
    s.synchronize()
    assert torch.equal(got, want)
    assert torch.equal(twice, want * 2)


def test_capture_replayed_twice_equals_eager():
    src, grid, shape = _inputs(3, 2, 730)
    eager = _push(src, grid, shape, DCT2, 3, general=True)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        _push(src, grid, shape, DCT2, 3, general=False)      # warm-up on the capture stream (allocator, kernel attributes)
    torch.cuda.current_stream(DEV).wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = _push(src, grid, shape, DCT2, 3, general=False)
    for it in range(2):
        out.fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager), it
    assert torch.equal(_push(src, grid, shape, DCT2, 3, general=False), eager)    # eager again behind the replays
