"""Owner-computes push (csrc/push_owner.hip): stray samples in shell bricks.

A sample tile that holds at most THIN_SHELL_RUN samples in shell bricks altogether publishes no run for them: own_bin scatters those
samples itself with float atomics (a wave per sample, a stencil tap per lane), and the shell launch of own_accumulate has nothing to do
unless a run was published.  INTERPOL_FLAG_SHELL_RUNS publishes every run (the behaviour before): both sides are run on the same inputs.

The lattice is (48, 40, 56): every dim >= 32, so dct2 / replicate / dct1 fold (interior first taps [lo, top) = [-9, n + 6)) and there
are 3 - 4 interior bricks per dim; under dft / zero nothing folds ([lo, top) = [0, n - K)) and a thick shell lies beside the strays.
The base field is the identity + sigma = 2 noise clamped to +-6 -- under a folding bound nothing of it reaches the shell -- and onto it
strays are planted at seeded samples: first taps at lo - 1, lo - 2, lo - 40, top, top + 1, top + 40 of each dim (from sample tiles at
that face of the sample grid: the tile's bricks stay within own_bin's local window, so the run is sorted, found to be one of a few and orphaned,
not just left unbinned), one stray out in all three dims, two strays of one tile in one shell brick, two strays of different tiles
with overlapping stencils.

The checker is the float64 oracle at the bar of tests/test_lean_kernels.py for paths with float atomics: rtol 1e-5 + 1e-5 max|ref|
(bf16 storage: the bar of the binned bf16 push of tests/test_hip_parity.py, 1e-2 + 1e-2 max|ref| against the oracle on the
bf16-rounded sources).  Outside the strays' stencils nothing but the colour launches writes: there the two sides agree bit for bit."""
import numpy as np
import pytest
import torch

import golden_util as G
import interpol
from oracle import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPLICATE, DCT1, DCT2, DFT, ZERO = 1, 2, 3, 6, 0
FOLDING = (REPLICATE, DCT1, DCT2)
SHAPE = (48, 40, 56)
TILE = 16                                   # own_bin: a workgroup bins a tile of 16^3 samples


def test_bound_codes():
    from interpol.codes import bound_to_code
    assert [bound_to_code(b) for b in ("replicate", "dct1", "dct2", "dft", "zero")] == [REPLICATE, DCT1, DCT2, DFT, ZERO]


def _orders(order):
    """Per-dim orders, and the orders the bricks see: a nearest-neighbour push runs as a trilinear one of the rounded coordinates."""
    o = list(order) if isinstance(order, (list, tuple)) else [order] * 3
    return o, [max(k, 1) for k in o]


def _limits(bound, k, n):
    """Interior first-tap cells [lo, top) of a dim (push_owner.hip: brick_grid)."""
    return (-9, n + 6) if bound in FOLDING and n >= 32 else (0, max(n - k, 0))


def _coord(ft, k, frac, nearest):
    """A coordinate whose first tap floor(x - (k - 1) / 2) is ft (nearest neighbour: whose rounded value is ft)."""
    return ft + (frac - 0.5) * 0.6 if nearest else ft + 0.5 * (k - 1) + frac


def _base(B, C, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    src = torch.randn([B, C, *SHAPE], generator=g).to(dtype)
    disp = (2.0 * torch.randn([B, *SHAPE, 3], generator=g)).clamp(-6.0, 6.0)
    return src, (interpol.identity_grid(SHAPE)[None] + disp).contiguous()


def _plant(grid, bound, order, seed):
    """Plants the strays into `grid` (CPU, in place) for every batch item; returns the samples (b, i, j, k) that were moved."""
    o, ko = _orders(order)
    nearest = o == [0, 0, 0]
    kb = [3] * 3 if len(set(ko)) > 1 else ko                # mixed orders: the cubic's bricks
    lim = [_limits(bound, kb[d], SHAPE[d]) for d in range(3)]
    rnd = np.random.RandomState(seed)
    moved = []

    def frac():
        return float(rnd.uniform(0.2, 0.8))

    def put(b, at, fts):
        """sample `at` of item b: the dims d of {d: first tap} move, the others keep the base field"""
        for d, ft in fts.items():
            grid[(b, *at, d)] = _coord(ft, ko[d], frac(), nearest)
        moved.append((b, *at))

    def face_sample(d, high):
        """a seeded sample of a tile at the low / high face of dim d"""
        at = [int(rnd.randint(4, SHAPE[e] - 4)) for e in range(3)]
        at[d] = int(rnd.randint(SHAPE[d] - 8, SHAPE[d])) if high else int(rnd.randint(0, TILE))
        return tuple(at)

    for b in range(grid.shape[0]):
        for d in range(3):
            lo, top = lim[d]
            for ft in (lo - 1, lo - 2, lo - 40):
                put(b, face_sample(d, False), {d: ft})
            for ft in (top, top + 1, top + 40):
                put(b, face_sample(d, True), {d: ft})
        # out in all three dims: below, above, below
        put(b, (2, SHAPE[1] - 3, 1), {0: lim[0][0] - 2, 1: lim[1][1] + 1, 2: lim[2][0] - 1})
        # two strays of ONE tile (samples 16 .. 31 of every dim) into ONE shell brick (first taps lo - 3 / lo - 5 of dim 0; the other
        # first taps 19 / 20 and 20 / 21: cells 28 .. 30 from lo = -9 or 19 .. 21 from lo = 0 -- one brick either way)
        put(b, (20, 20, 20), {0: lim[0][0] - 3, 1: 19, 2: 20})
        put(b, (21, 22, 23), {0: lim[0][0] - 5, 1: 20, 2: 21})
        # two strays of DIFFERENT tiles (dim 1: samples 0 .. 15 and 16 .. 31) whose stencils overlap
        put(b, (3, 12, 20), {0: lim[0][0] - 1, 1: 17, 2: 25})
        put(b, (3, 20, 20), {0: lim[0][0] - 2, 1: 18, 2: 26})
    return sorted(set(moved))


_INPUTS = {}


def _inputs(B, C, bound, order, seed, dtype=torch.float32):
    """(src, grid on the device, src, grid on the CPU, strays), built once per key."""
    key = (B, C, bound, str(order), seed, dtype)
    if key not in _INPUTS:
        src, grid = _base(B, C, seed, dtype)
        strays = _plant(grid, bound, order, seed + 1)
        _INPUTS[key] = (src.to(DEV), grid.to(DEV), src, grid, strays)
    return _INPUTS[key]


def _oracle(fn, *args):
    oracle.set_threads(8)
    try:
        return np.asarray(fn(*args))
    finally:
        oracle.set_threads(1)


_WANT = {}


def _oracle_push(src, grid, bound, order):
    """float64 reference, computed once per input pair (the tensors of _inputs live as long as the module)."""
    key = (id(src), id(grid), bound, str(order))
    if key not in _WANT:
        _WANT[key] = (src, grid, _oracle(oracle.grid_push, src.double(), grid.double(), list(SHAPE), [bound], _orders(order)[0], 1))
    return _WANT[key][2]


def _push(src, grid, bound, order, shell_runs=False, serial=False, flags=0, **kw):
    from interpol import _hip
    fl = _hip.FLAG_BINNED_SCATTER | flags
    if shell_runs:
        fl |= _hip.FLAG_SHELL_RUNS
    if serial:
        fl |= _hip.FLAG_SERIAL_ITEMS
    return _hip.scatter("push", src, grid, list(SHAPE), [bound] * 3, _orders(order)[0], 1, flags=fl, **kw)


def _close(got, want, what):
    G.assert_close(got.double().cpu().numpy(), want, 1e-5, 1e-5, what)


# ---- case 1: strays against the oracle -- a chosen set, not the full product: every bound with the cubic, every order with dct2 and
# with dft, C and the count channel and B (one chain; two chains of one and two items; two chains of two items) spread over them
CASES1 = [
    # bound, order, B, C, with_count
    (DCT2, 3, 4, 2, False),
    (DCT2, 3, 1, 1, True),
    (DCT2, 2, 3, 3, False),
    (DCT2, 1, 3, 2, True),
    (DCT2, (1, 3, 2), 4, 2, False),
    (DCT2, 0, 3, 1, False),
    (REPLICATE, 3, 3, 3, True),
    (REPLICATE, 0, 1, 2, False),
    (DCT1, 3, 4, 1, False),
    (DCT1, 2, 1, 2, True),
    (DFT, 3, 3, 2, False),
    (DFT, 2, 4, 1, True),
    (DFT, 1, 1, 3, False),
    (DFT, (1, 3, 2), 3, 2, False),
    (DFT, 0, 4, 2, False),
    (ZERO, 3, 4, 2, True),
    (ZERO, 1, 3, 1, False),
    (ZERO, (1, 3, 2), 1, 3, True),
]


@pytest.mark.parametrize("serial", [False, True])
@pytest.mark.parametrize("bound,order,B,C,with_count", CASES1)
def test_strays_against_the_oracle(bound, order, B, C, with_count, serial):
    src, grid, src_c, grid_c, strays = _inputs(B, C, bound, order, 1000 + 7 * B + C)
    assert len(strays) >= 20 * B
    got = _push(src, grid, bound, order, serial=serial, with_count=with_count)
    want = _oracle_push(src_c, grid_c, bound, order)
    if with_count:
        cnt = _oracle(oracle.grid_count, grid_c.double(), list(SHAPE), [bound], _orders(order)[0], 1)
        assert got.shape[1] == C + 1
        _close(got[:, C:], cnt.reshape(B, 1, *SHAPE), ("count channel", bound, order, B, C, serial))
    _close(got[:, :C], want, ("strays", bound, order, B, C, with_count, serial))


# ---- case 2: the default against INTERPOL_FLAG_SHELL_RUNS
@pytest.mark.parametrize("bound", [DCT2, REPLICATE, DCT1])
def test_default_equals_published_runs_outside_the_strays(bound):
    """Under a folding bound only the strays leave the interior bricks.  Their footprint: where an oracle push of unit sources at the
    strays alone (zero elsewhere) is non-zero.  Outside it the colour launches alone write, on both sides: bit for bit.  Inside it
    float atomics take part on both sides: the bar."""
    B, C = 3, 2
    src, grid, src_c, grid_c, strays = _inputs(B, C, bound, 3, 2000 + bound)
    a = _push(src, grid, bound, 3)
    b = _push(src, grid, bound, 3, shell_runs=True)
    unit = torch.zeros([B, 1, *SHAPE], dtype=torch.float64)
    for s in strays:
        unit[(s[0], 0, *s[1:])] = 1.0
    foot = torch.from_numpy(_oracle_push(unit, grid_c, bound, 3) != 0).expand(B, C, *SHAPE).to(DEV)
    assert 0 < int(foot.sum()) < foot.numel() // 4
    assert float(b.abs().max()) > 0
    assert torch.equal(a[~foot], b[~foot]), bound
    G.assert_close(a[foot].double().cpu().numpy(), b[foot].double().cpu().numpy(), 1e-5, 1e-5, ("inside the footprint", bound))
    _close(a, _oracle_push(src_c, grid_c, bound, 3), ("default", bound))


# ---- case 3: the threshold from both sides, whatever its value
@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 300])
def test_n_strays_of_one_tile_in_one_shell_brick(n):
    """n samples of the sample tile at the origin land in the shell brick below the first interior brick of dim 0 (first taps
    [lo - 14, lo - 2) there, [lo + 2, lo + 14) in the other dims)."""
    B, C = 2, 2
    src, grid = _base(B, C, 3000)
    rnd = np.random.RandomState(3000 + n)
    lo = -9
    for b in range(B):
        picks = rnd.permutation(TILE ** 3)[:n]
        for s in picks:
            at = (int(s) // 256, (int(s) // 16) % 16, int(s) % 16)
            for d in range(3):
                grid[(b, *at, d)] = (lo - 14 if d == 0 else lo + 2) + 1.0 + float(rnd.uniform(0.0, 12.0))
    got = _push(src.to(DEV), grid.to(DEV), DCT2, 3)
    _close(got, _oracle_push(src, grid, DCT2, 3), ("n strays", n))


# ---- case 4: thick shell
@pytest.mark.parametrize("shell_runs", [False, True])
def test_thick_shell_of_a_zoom(shell_runs):
    """Zoom 1.5 about the centre under dct2: up to a quarter of the lattice beyond every face, thick runs with a thin fringe."""
    B, C = 3, 2
    key = ("zoom",)
    if key not in _INPUTS:
        src, grid = _base(B, C, 4000)
        c = torch.tensor([(n - 1) / 2 for n in SHAPE])
        ident = interpol.identity_grid(SHAPE)[None]
        grid = (c + 1.5 * (ident - c) + (grid - ident)).contiguous()
        _INPUTS[key] = (src.to(DEV), grid.to(DEV), _oracle_push(src, grid, DCT2, 3))
    src, grid, want = _INPUTS[key]
    _close(_push(src, grid, DCT2, 3, shell_runs=shell_runs), want, ("zoom 1.5", shell_runs))


# ---- case 5: remaining variants
def test_accumulate_into_a_nonzero_target():
    from interpol import _hip
    src, grid, src_c, grid_c, _ = _inputs(3, 2, DCT2, 3, 5000)
    base = torch.randn([3, 2, *SHAPE], generator=torch.Generator().manual_seed(5))
    out = base.to(DEV)
    _push(src, grid, DCT2, 3, flags=_hip.FLAG_ACCUMULATE, out=out)
    _close(out, base.double().numpy() + _oracle_push(src_c, grid_c, DCT2, 3), "accumulate")


def test_target_shared_by_the_batch_items():
    src, grid, src_c, grid_c, _ = _inputs(4, 2, DCT2, 3, 5100)
    got = _push(src, grid, DCT2, 3, shared=True)
    assert got.shape[0] == 1
    _close(got, _oracle_push(src_c, grid_c, DCT2, 3).sum(0, keepdims=True), "shared target")


def test_bf16_storage():
    src, grid, src_c, grid_c, _ = _inputs(3, 2, DCT2, 3, 5200, dtype=torch.bfloat16)
    got = _push(src, grid, DCT2, 3)
    assert got.dtype == torch.bfloat16
    G.assert_close(got.double().cpu().numpy(), _oracle_push(src_c, grid_c, DCT2, 3), 1e-2, 1e-2, "bf16 storage")


def test_non_default_stream():
    src, grid, src_c, grid_c, _ = _inputs(3, 2, DCT2, 3, 5300)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        got = _push(src, grid, DCT2, 3)
        twice = got * 2                                     # a consumer on the caller's stream, right behind the call
    s.synchronize()
    want = _oracle_push(src_c, grid_c, DCT2, 3)
    _close(got, want, "side stream")
    _close(twice, 2 * want, "side stream, consumer")


def test_capture_replayed_twice():
    src, grid, src_c, grid_c, _ = _inputs(3, 2, DCT2, 3, 5400)
    want = _oracle_push(src_c, grid_c, DCT2, 3)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        _push(src, grid, DCT2, 3)                           # warm-up on the capture stream (allocator, kernel attributes)
    torch.cuda.current_stream(DEV).wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = _push(src, grid, DCT2, 3)
    for it in range(2):
        out.fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        _close(out, want, ("replay", it))


# ---- case 6: grid_count
@pytest.mark.parametrize("bound", [DCT2, DFT])
def test_count_with_strays(bound):
    from interpol import _hip
    _, grid, _, grid_c, _ = _inputs(3, 2, bound, 3, 6000 + bound)
    got = _hip.scatter("count", None, grid, list(SHAPE), [bound] * 3, [3] * 3, 1, flags=_hip.FLAG_BINNED_SCATTER)
    want = _oracle(oracle.grid_count, grid_c.double(), list(SHAPE), [bound], [3], 1)
    _close(got, want.reshape(got.shape), ("count", bound))


# ---- case 7: the flag
def test_flag_value_and_api_never_sets_it(monkeypatch):
    """Bit 28, outside the other flags and the debug bits (8 - 23); the Python API (grid_push, grid_count and the backward of
    grid_pull, which pushes) never hands it to _hip.scatter."""
    from interpol import _hip
    assert _hip.FLAG_SHELL_RUNS == 1 << 28
    assert not _hip.FLAG_SHELL_RUNS & (_hip.FLAG_GENERAL_KERNELS | _hip.FLAG_SERIAL_ITEMS | _hip.FLAG_AUTO_SCATTER | _hip.FLAG_SMALL_TILES | 0xffffff)
    seen = []
    real = _hip.scatter

    def spy(*a, **kw):
        seen.append(int(kw.get("flags", a[7] if len(a) > 7 else 0)))
        return real(*a, **kw)
    monkeypatch.setattr(_hip, "scatter", spy)
    src, grid, _, _, _ = _inputs(2, 2, DCT2, 3, 7000)
    src = src.clone().requires_grad_(True)
    interpol.grid_push(src, grid, list(SHAPE), interpolation=3, bound="dct2", extrapolate=True).sum().backward()
    interpol.grid_count(grid, list(SHAPE), interpolation=3, bound="dct2", extrapolate=True)
    x = src.detach().clone().requires_grad_(True)
    interpol.grid_pull(x, grid, interpolation=3, bound="dct2", extrapolate=True).sum().backward()
    assert len(seen) >= 2, seen
    assert not any(f & _hip.FLAG_SHELL_RUNS for f in seen), seen
