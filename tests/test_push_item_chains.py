"""Owner-computes push (csrc/push_owner.hip): the batch items as concurrent stream chains against the single-stream schedule
(INTERPOL_FLAG_SERIAL_ITEMS) on the same inputs.

The schedule changes WHEN a brick of an item is accumulated, never what is added to it: inside a brick the sums are integers and
the up to eight boxes that meet at a lattice point are added in the fixed order of the colours of their own item.  So wherever the
single-stream schedule is bit-reproducible (dct2 / replicate / dct1, every stencil within 9 points of the lattice: no shell launch,
no direct scatter -- push_owner.hip, head of the file) the two schedules must agree bit for bit: torch.equal.  Where float atomics
take part (the shell launch under dft, samples far outside the lattice) neither schedule is reproducible against itself; each is
then compared with the float64 oracle at the bar of the owner tests of test_hip_parity.py (rtol 1e-5 + 1e-5 max|ref|)."""
import numpy as np
import pytest
import torch

import golden_util as G
import interpol
from oracle import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DCT2, REPLICATE, DCT1, DFT = 3, 1, 2, 6


def test_bound_codes():
    from interpol.codes import bound_to_code
    assert [bound_to_code(b) for b in ("dct2", "replicate", "dct1", "dft")] == [DCT2, REPLICATE, DCT1, DFT]


def _inputs(B, C, n, seed, amp=6.0, sigma=2.0, dtype=torch.float32):
    """Sources and a dense grid: identity + i.i.d. noise of `sigma` voxels, clamped to +-amp (amp <= 6: every stencil of a cubic
    stays within 9 points of the lattice -- nothing reaches the shell bricks or the direct scatter)."""
    g = torch.Generator().manual_seed(seed)
    shape = (n, n - 16, n + 8)
    src = torch.randn([B, C, *shape], generator=g).to(dtype)
    disp = sigma * torch.randn([B, *shape, 3], generator=g)
    if amp is not None:
        disp = disp.clamp(-amp, amp)
    grid = (interpol.identity_grid(shape)[None] + disp).contiguous()
    return src.to(DEV), grid.to(DEV), list(shape)


def _push(src, grid, shape, bound, order, serial, flags=None, **kw):
    from interpol import _hip
    fl = _hip.FLAG_BINNED_SCATTER if flags is None else flags
    if serial:
        fl |= _hip.FLAG_SERIAL_ITEMS
    order = order if isinstance(order, (list, tuple)) else [order] * 3
    return _hip.scatter("push", src, grid, shape, [bound] * 3, list(order), 1, flags=fl, **kw)


@pytest.mark.parametrize("B", [1, 2, 3, 4, 5, 9])
def test_chains_equal_serial_over_batch_sizes(B):
    """More items than chains, uneven item ranges, a single item (no fork)."""
    src, grid, shape = _inputs(B, 2, 96, 100 + B)
    a = _push(src, grid, shape, DCT2, 3, serial=False)
    b = _push(src, grid, shape, DCT2, 3, serial=True)
    assert float(b.abs().max()) > 0
    assert torch.equal(a, b), B


@pytest.mark.parametrize("C", [1, 2, 3])
@pytest.mark.parametrize("with_count", [False, True])
def test_chains_equal_serial_channels_and_count(C, with_count):
    src, grid, shape = _inputs(3, C, 96, 200 + C)
    a = _push(src, grid, shape, REPLICATE, 3, serial=False, with_count=with_count)
    b = _push(src, grid, shape, REPLICATE, 3, serial=True, with_count=with_count)
    assert a.shape[1] == C + int(with_count)
    assert torch.equal(a, b), (C, with_count)


@pytest.mark.parametrize("order", [1, 2, 3, (1, 3, 2)])
def test_chains_equal_serial_orders(order):
    src, grid, shape = _inputs(4, 2, 96, 300)
    a = _push(src, grid, shape, DCT1, order, serial=False)
    b = _push(src, grid, shape, DCT1, order, serial=True)
    assert torch.equal(a, b), order


def test_chains_equal_serial_count_and_default_routing():
    """interpol_count (one channel, no sources) and the probe-routed default (INTERPOL_FLAG_AUTO_SCATTER: the gate is written once,
    in front of the fork)."""
    from interpol import _hip
    src, grid, shape = _inputs(4, 2, 96, 350)
    ca = _hip.scatter("count", None, grid, shape, [DCT2] * 3, [3] * 3, 1, flags=_hip.FLAG_BINNED_SCATTER)
    cb = _hip.scatter("count", None, grid, shape, [DCT2] * 3, [3] * 3, 1, flags=_hip.FLAG_BINNED_SCATTER | _hip.FLAG_SERIAL_ITEMS)
    assert torch.equal(ca, cb)
    a = _push(src, grid, shape, DCT2, 3, serial=False, flags=_hip.FLAG_AUTO_SCATTER)
    b = _push(src, grid, shape, DCT2, 3, serial=True, flags=_hip.FLAG_AUTO_SCATTER)
    assert torch.equal(a, b)
    assert torch.equal(a, _push(src, grid, shape, DCT2, 3, serial=True))     # (sigma = 2, two channels: the probe gives the call to the bricks)


def test_chains_equal_serial_accumulate():
    """INTERPOL_FLAG_ACCUMULATE: no zero-fill, the chains add into what the target holds."""
    from interpol import _hip
    src, grid, shape = _inputs(3, 2, 96, 360)
    base = torch.randn([3, 2, *shape], generator=torch.Generator().manual_seed(5)).to(DEV)
    a, b = base.clone(), base.clone()
    _push(src, grid, shape, DCT2, 3, serial=False, flags=_hip.FLAG_BINNED_SCATTER | _hip.FLAG_ACCUMULATE, out=a)
    _push(src, grid, shape, DCT2, 3, serial=True, flags=_hip.FLAG_BINNED_SCATTER | _hip.FLAG_ACCUMULATE, out=b)
    assert not torch.equal(a, base)
    assert torch.equal(a, b)


def test_chains_equal_serial_bf16():
    """bf16 sources: the chains fill a float accumulator in the scratch buffer, the narrowing runs behind the join."""
    src, grid, shape = _inputs(4, 2, 96, 400, dtype=torch.bfloat16)
    a = _push(src, grid, shape, DCT2, 3, serial=False)
    b = _push(src, grid, shape, DCT2, 3, serial=True)
    assert a.dtype == torch.bfloat16 and float(b.float().abs().max()) > 0
    assert torch.equal(a, b)


def test_shared_target_stays_serial():
    """One target for all items (batch stride 0): the items meet in the same bricks, there is nothing to run side by side."""
    src, grid, shape = _inputs(4, 2, 96, 500)
    a = _push(src, grid, shape, DCT2, 3, serial=False, shared=True)
    b = _push(src, grid, shape, DCT2, 3, serial=True, shared=True)
    assert a.shape[0] == 1
    assert torch.equal(a, b)


def test_chains_on_a_side_stream_of_the_caller():
    src, grid, shape = _inputs(4, 2, 96, 600)
    want = _push(src, grid, shape, DCT2, 3, serial=True)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        got = _push(src, grid, shape, DCT2, 3, serial=False)
        twice = got * 2                                    # a consumer on the caller's stream, right behind the join
    s.synchronize()
    assert torch.equal(got, want)
    assert torch.equal(twice, want * 2)


def test_back_to_back_calls_share_a_workspace():
    """Two calls through ONE scratch buffer with no synchronisation in between, then a consumer kernel on the stream: the second
    call's own_zero must come behind every chain of the first (join), the consumer behind every chain of the second."""
    import ctypes
    from interpol import _hip
    src1, grid1, shape = _inputs(4, 2, 96, 700)
    src2, grid2, _ = _inputs(4, 2, 96, 701)
    want1 = _push(src1, grid1, shape, DCT2, 3, serial=True)
    want2 = _push(src2, grid2, shape, DCT2, 3, serial=True)
    L = _hip.lib()
    B, C = 4, 2
    out1 = torch.full([B, C, *shape], 7.0, device=DEV)
    out2 = torch.full([B, C, *shape], 7.0, device=DEV)

    def problem(src, grid, vol):
        return _hip.make_problem(3, torch.float32, torch.float32, [DCT2] * 3, [3] * 3, 1, B, C, shape, shape,
                                 [vol.stride(0), vol.stride(1)] + [vol.stride(2 + d) for d in range(3)], _hip._grid_strides(grid, B, 3),
                                 [src.stride(0), src.stride(1)] + [src.stride(2 + d) for d in range(3)] + [0, 0], _hip.FLAG_BINNED_SCATTER)
    p1, p2 = problem(src1, grid1, out1), problem(src2, grid2, out2)
    nbytes = int(L.interpol_scatter_workspace(ctypes.byref(p1), 0))
    assert nbytes > 0 and nbytes == int(L.interpol_scatter_workspace(ctypes.byref(p2), 0))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    st = _hip._stream(torch.device(DEV))
    with torch.cuda.device(DEV):
        rc1 = L.interpol_push(ctypes.byref(p1), _hip._ptr(src1), _hip._ptr(grid1), _hip._ptr(out1), _hip._ptr(ws), nbytes, st)
        rc2 = L.interpol_push(ctypes.byref(p2), _hip._ptr(src2), _hip._ptr(grid2), _hip._ptr(out2), _hip._ptr(ws), nbytes, st)
        total = out1 + out2
    torch.cuda.synchronize()
    assert rc1 == 0 and rc2 == 0
    assert torch.equal(out1, want1) and torch.equal(out2, want2)
    assert torch.equal(total, want1 + want2)


def test_capture_is_serial_and_equals_eager():
    """Under torch.cuda.graph the call keeps to the captured stream (a captured graph has no parallel branches); replayed twice,
    it equals the eager call, which runs the chains."""
    src, grid, shape = _inputs(4, 2, 96, 800)
    eager = _push(src, grid, shape, DCT2, 3, serial=False)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        _push(src, grid, shape, DCT2, 3, serial=False)      # warm-up on the capture stream (allocator, kernel attributes)
    torch.cuda.current_stream(DEV).wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = _push(src, grid, shape, DCT2, 3, serial=False)
    for it in range(2):
        out.fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager), it
    assert torch.equal(_push(src, grid, shape, DCT2, 3, serial=False), eager)    # eager again behind the replays


@pytest.mark.parametrize("serial", [False, True])
def test_rough_field_reaches_the_shell(serial):
    """sigma = 9 under dft: the stencils that wrap go to the shell launch (global float atomics), every chain runs its own.  Both
    schedules against the float64 oracle, at the bar of the shared-target owner test."""
    B, C, n = 3, 2, 96
    src, grid, shape = _inputs(B, C, n, 900, amp=None, sigma=9.0)
    got = _push(src, grid, shape, DFT, 3, serial=serial)
    oracle.set_threads(8)
    try:
        want = np.asarray(oracle.grid_push(src.cpu().double(), grid.cpu().double(), shape, [DFT], [3], 1))
    finally:
        oracle.set_threads(1)
    G.assert_close(got.cpu().numpy(), want, 1e-5, 1e-5, ("rough dft push", serial))


@pytest.mark.parametrize("serial", [False, True])
def test_samples_far_outside_take_the_direct_scatter(serial):
    """dct2 with a tenth of the samples thrown up to 400 voxels off the lattice: beyond the binned range own_bin scatters them itself
    with float atomics -- into a slice of the target that its own chain has zeroed before."""
    B, C, n = 3, 2, 96
    src, grid, shape = _inputs(B, C, n, 950)
    gen = torch.Generator().manual_seed(951)
    far = (torch.rand(grid.shape[:-1], generator=gen) < 0.1).to(DEV)
    grid = torch.where(far[..., None], grid + 400.0 * (torch.rand(grid.shape, generator=gen).to(DEV) - 0.5) * 2, grid).contiguous()
    got = _push(src, grid, shape, DCT2, 3, serial=serial)
    oracle.set_threads(8)
    try:
        want = np.asarray(oracle.grid_push(src.cpu().double(), grid.cpu().double(), shape, [DCT2], [3], 1))
    finally:
        oracle.set_threads(1)
    G.assert_close(got.cpu().numpy(), want, 1e-5, 1e-5, ("far samples", serial))
