"""The five prefilter kernels (csrc/prefilter.hip) against the float64 oracle, one test id per kernel organisation and case:

    wave_full   inner == 1, n in {256, 512, 1024, 2048}, a short leading initial sum      prefilter_wave_full
    wave        inner == 1, every other n <= 2048 (and the four n under dft)              prefilter_wave
    tile        inner >= 16 at the four n, a short leading initial sum                    prefilter_tile (16-bit: twice the lines)
    strided     inner >= 16, every other n (and the four n under dft)                     prefilter_strided
    serial      inner 2..15, or inner == 1 with n > 2048                                  prefilter_serial

`organisation()` restates the dispatch of launch_filter_t (prefilter.hip:602-649) so that every id is named after the kernel it
runs.  "A short leading initial sum" (`lead`) excludes dft and a dct1 line no longer than the initial sum's horizon
ceil(-30 / log|pole|) (filter_params.hpp:41-49): 18, 23, 30, 36, 42, 49 points for orders 2..7, so at the four n only dft is excluded.

The first test keeps every (n, inner, order, bound, dtype) of the former test_prefilter_kernels_against_oracle of
tests/test_hip_parity.py at its tolerances (float64 1e-10, float32 1e-5 of max|ref|), one id per (dtype, inner, n, order); the
five bounds of an id are all run before it reports, so a failure names every bad case.

16-bit storage: the reference is the float64 oracle on the rounded input, the bar the one of tests/fuzz_oracle_prefilter.py,
3e-2 (1 + 2 [order >= 2]) of max|ref| per filtered dim, for bf16 and f16.  f16 runs orders 2..5: the gain of orders 6 and 7 (about
5e3) puts the per-pass intermediates of unit-scale inputs near the format's range.
Every case prints `PARITY ...`; `python tests/separable_truth.py` condenses a `-s` log into profiles/separable_parity.txt."""
import math

import numpy as np
import pytest
import torch

import interpol
from oracle import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = {"f32": torch.float32, "f64": torch.float64, "bf16": torch.bfloat16, "f16": torch.float16}
BOUNDS = (0, 1, 2, 3, 6)                        # zero (-> dct1), replicate (-> dct2), dct1, dct2, dft
NAMES = {0: "zero", 1: "replicate", 2: "dct1", 3: "dct2", 4: "dst1", 5: "dst2", 6: "dft"}
FULL_N = (256, 512, 1024, 2048)                 # 64 * RPL, RPL in 4, 8, 16, 32: the lines that fill a wave (prefilter.hip:609, 625-628)
_X = {}


def _poles(order):
    """Poles of the B-spline of `order`: the roots inside the unit circle of the polynomial of its samples at the integers."""
    h = (order + 1) // 2
    b = [oracle.weight(order, float(abs(k))) for k in range(-h, h + 1)]
    while b[0] == 0:
        b = b[1:-1]
    return sorted((r.real for r in np.roots(b) if abs(r) < 1), key=abs, reverse=True)


HORIZON = {o: max(math.ceil(-30. / math.log(abs(p))) for p in _poles(o)) for o in range(2, 8)}      # filter_params.hpp:41


def organisation(n, inner, bound, order, dt):
    """launch_filter_t, prefilter.hip:602-649."""
    lead = dt != "f64" and bound != 6 and not (bound in (0, 2) and n <= HORIZON[order])
    if inner == 1 and lead and n in FULL_N:
        return "wave_full"
    if inner >= 16 and lead and n in FULL_N:
        return "tile"
    if inner == 1 and 2 <= n <= 2048:
        return "wave"
    return "strided" if inner >= 16 else "serial"


def tile_lines(n, dt):
    """Lines per LDS tile of prefilter_tile (prefilter.hip:624-628)."""
    return {256: 64, 512: 64, 1024: 32, 2048: 16}[n] * (2 if dt in ("bf16", "f16") else 1)


def _input(shape, dt, seed):
    """Unit-scale input as stored in `dt` on the device, and the same values in float64 numpy."""
    key = (tuple(shape), dt, seed)
    if key not in _X:
        x = torch.randn(list(shape), generator=torch.Generator().manual_seed(seed), dtype=torch.float64).to(DT[dt])
        _X[key] = (x.to(DEV), x.double().numpy())
    return _X[key]


def _bar(dt, orders):
    k = sum(o >= 2 for o in orders)
    return {"f32": 2e-5, "f64": 1e-12, "bf16": 3e-2, "f16": 3e-2}[dt] * (1 + 2 * k)       # tests/fuzz_oracle_prefilter.py:37


def _err(got, want):
    return float(np.abs(got.double().cpu().numpy() - want).max() / max(np.abs(want).max(), 1e-30))


def _run_line(shape, dt, order, bounds, tol, org, seed=0):
    """spline_coeff along dim 1 of (outer, n, inner), out of place and in place, against the oracle: every bound runs, every
    miss is reported."""
    xd, x64 = _input(shape, dt, seed)
    keep = xd.clone()
    bad, worst = [], 0.0
    for bound in bounds:
        if org is not None:
            assert organisation(shape[1], shape[2], bound, order, dt) == org, (shape, bound, order, dt)
        want = np.asarray(oracle.spline_coeff(x64, bound, order, dim=1))
        out = interpol.spline_coeff(xd, interpolation=order, bound=NAMES[bound], dim=1)
        assert out.dtype == DT[dt] and out.data_ptr() != xd.data_ptr() and torch.equal(xd, keep), (shape, bound, "source modified")
        work = xd.clone()
        inp = interpol.spline_coeff(work, interpolation=order, bound=NAMES[bound], dim=1, inplace=True)
        assert inp.data_ptr() == work.data_ptr()
        for how, got in (("out of place", out), ("in place", inp)):
            err = _err(got, want)
            worst = max(worst, err)
            if not err < tol:
                bad.append((shape, dt, order, NAMES[bound], how, "%.3e" % err))
    print("PARITY prefilter %s %s %d %.3e" % (org or "legacy", dt, order, worst))
    assert not bad, bad


# ---------------------------------------------------------------------------
# every case of the former test_prefilter_kernels_against_oracle
# ---------------------------------------------------------------------------
LEGACY_N = (2, 3, 5, 17, 64, 65, 127, 128, 200, 256, 512, 1000, 1024, 2048, 2500)


@pytest.mark.parametrize("order", range(2, 8))
@pytest.mark.parametrize("n", LEGACY_N)
@pytest.mark.parametrize("inner", [1, 16, 33, 3])
@pytest.mark.parametrize("dt,tol", [("f64", 1e-10), ("f32", 1e-5)])
def test_prefilter_kernels_against_oracle(dt, tol, inner, n, order):
    _run_line((3, n, inner), dt, order, BOUNDS, tol, None, seed=2024 + inner)


# ---------------------------------------------------------------------------
# one id per kernel organisation
# ---------------------------------------------------------------------------
def _organisation_cases():
    """(organisation, (outer, n, inner), dtype, order, bounds): the shapes of each organisation, their bounds grouped by the
    kernel that serves them."""
    shapes = ([(5, n, 1) for n in FULL_N + (2, 3, 63, 64, 65, 129, 2047, 2500)]                 # wave_full | wave | serial
              + [(3, n, 33) for n in FULL_N + (2, 3, 63, 65, 129, 2047, 2500)]                  # tile | strided
              + [(2, n, 16) for n in (256, 2048, 129)]
              + [(3, n, i) for n, i in ((256, 2), (129, 15), (2047, 7), (2048, 3), (65, 3))])   # serial
    out = []
    for shape in shapes:
        for dt in DT:
            for order in range(2, 6 if dt == "f16" else 8):
                groups = {}
                for b in BOUNDS:
                    groups.setdefault(organisation(shape[1], shape[2], b, order, dt), []).append(b)
                out += [(org, shape, dt, order, tuple(bs)) for org, bs in groups.items()]
    return out


def _tol(dt):
    return {"f64": 1e-10, "f32": 1e-5, "bf16": _bar("bf16", [2]), "f16": _bar("f16", [2])}[dt]


@pytest.mark.parametrize("org,shape,dt,order,bounds", _organisation_cases(),
                         ids=["%s-%dx%dx%d-%s-k%d-b%s" % ((c[0],) + c[1] + (c[2], c[3], "".join(map(str, c[4])))) for c in _organisation_cases()])
def test_organisation(org, shape, dt, order, bounds):
    _run_line(shape, dt, order, bounds, _tol(dt), org, seed=11)


# ---------------------------------------------------------------------------
# tiles: a full tile, several tiles, a ragged last one, one and several outer slices
# ---------------------------------------------------------------------------
def _tile_cases():
    out, i = [], 0
    for inner in (64, 70, 130, 260):
        for outer in (1, 3):
            for n in FULL_N:
                for dt in ("f32", "bf16", "f16"):
                    orders = (2 + i % 4, 6 + i % 2) if dt != "f16" else (2 + i % 4,)
                    out += [((outer, n, inner), dt, o) for o in orders]
                    i += 1
    return out


@pytest.mark.parametrize("shape,dt,order", _tile_cases(), ids=str)
def test_tiles(shape, dt, order):
    _run_line(shape, dt, order, (0, 1, 2, 3), _tol(dt), "tile", seed=12)


# ---------------------------------------------------------------------------
# what `lead` keeps out of the lean kernels: dft at the four n, dct1 lines at and below the horizon of the initial sum
# ---------------------------------------------------------------------------
def _dtype_orders():
    return [(dt, order) for dt in DT for order in range(2, 6 if dt == "f16" else 8)]


@pytest.mark.parametrize("dt,order", _dtype_orders())
@pytest.mark.parametrize("inner,outer", [(1, 5), (33, 3), (64, 2)])
def test_dft_goes_to_the_general_kernels(inner, outer, dt, order):
    for n in FULL_N:
        _run_line((outer, n, inner), dt, order, (6,), _tol(dt), "wave" if inner == 1 else "strided", seed=13)


@pytest.mark.parametrize("dt,order", _dtype_orders())
@pytest.mark.parametrize("inner,org", [(1, "wave"), (33, "strided"), (3, "serial")])
def test_dct1_at_and_below_the_horizon(inner, org, dt, order):
    for n in (HORIZON[order] - 1, HORIZON[order], HORIZON[order] + 1):        # full initial sum, full, truncated
        _run_line((4, n, inner), dt, order, (0, 2), _tol(dt), org, seed=14)


# ---------------------------------------------------------------------------
# spline_coeff_nd: 2 and 3 filtered dims under 0 - 2 leading dims, mixed orders and bounds per dim
# ---------------------------------------------------------------------------
def _nd_cases():
    out, i = [], 0
    for shape in ((2, 3, 65, 256), (3, 256, 33), (2, 17, 64, 70), (4, 1, 256)):
        for nd in (2, 3):
            for dt in DT:
                hi = 5 if dt == "f16" else 7
                orders = [[3, 2, hi], [hi, 0, 4], [2, 5, 1], [4, 3, 3]][(i + i // 4) % 4][-nd:]      # (every dtype meets every mix)
                bounds = [BOUNDS[(i + i // 4 + d) % 5] for d in range(nd)]
                out.append((shape, nd, dt, tuple(orders), tuple(bounds)))
                i += 1
    return out


@pytest.mark.parametrize("shape,nd,dt,orders,bounds", _nd_cases(), ids=str)
def test_spline_coeff_nd(shape, nd, dt, orders, bounds):
    xd, x64 = _input(shape, dt, 15)
    want = np.asarray(oracle.spline_coeff_nd(x64, list(bounds), list(orders), dim=nd))
    out = interpol.spline_coeff_nd(xd, list(orders), [NAMES[b] for b in bounds], nd)
    work = xd.clone()
    inp = interpol.spline_coeff_nd(work, list(orders), [NAMES[b] for b in bounds], nd, inplace=True)
    assert inp.data_ptr() == work.data_ptr() and out.data_ptr() != xd.data_ptr() and out.dtype == DT[dt]
    tol = _bar(dt, orders)
    errs = {"out of place": _err(out, want), "in place": _err(inp, want)}
    print("PARITY prefilter nd%d %s %d %.3e" % (nd, dt, max(orders), max(errs.values())))
    assert all(e < tol for e in errs.values()), (shape, nd, dt, orders, bounds, errs, tol)
    if 1 in shape[-nd:]:                        # a line of one point is its own coefficient
        d = len(shape) - nd + shape[-nd:].index(1)
        rest = [(o, b) for k, (o, b) in enumerate(zip(orders, bounds)) if len(shape) - nd + k != d]
        alone = oracle.spline_coeff_nd(np.squeeze(x64, d), [b for _, b in rest], [o for o, _ in rest], dim=nd - 1)
        assert np.array_equal(np.squeeze(want, d), np.asarray(alone))


# ---------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bound", ["dst1", "dst2"])
def test_dst_bounds_raise_from_order_two(bound):
    x = torch.randn(3, 65, 4, device=DEV)
    for order in range(2, 8):
        with pytest.raises(NotImplementedError):
            interpol.spline_coeff(x, interpolation=order, bound=bound, dim=1)
        with pytest.raises(NotImplementedError):
            interpol.spline_coeff_nd(x, interpolation=[1, order], bound=["dct2", bound], dim=2)
    for order in (0, 1):                        # (no filter to run: the identity, as in the reference)
        assert torch.equal(interpol.spline_coeff(x, interpolation=order, bound=bound, dim=1), x)
