"""The bar of tests/storage_contract.py does its job before a GPU sees it: a single round-to-nearest-even of the truth stays inside it
with no element excluded, and each way a 16-bit kernel goes wrong -- truncation, two roundings, a 16-bit partial sum, flushed f16
subnormals -- lands outside it on at least a tenth of the elements.  No GPU.

Vectors: 2e5 float64 values, magnitudes log-uniform over 1e-6 .. 1e3, both signs (f16: the subnormal range 2^-24 .. 2^-14 as well).
`scale` of the bar is max|want| OF A CALL, and the outputs of one call do not span nine decades: the vector is judged decade by
decade, each decade a call with its own max|want| (`_bands`).  The reference is held inside the bar both ways -- per decade and as one
call over the whole vector.

Round half away from zero: at an exact tie both neighbours are half an ulp off, so no bar on |got - want| can tell them apart -- the
test asserts that (ratio <= 1) and that the bit-for-bit comparison, which the tie cases of tests/test_storage_contract_gpu.py use,
catches every tie whose neighbour towards zero is even."""
import numpy as np
import pytest
import torch

import storage_contract as SC

N = 200000
DT = {"bf16": torch.bfloat16, "f16": torch.float16}
TYPES = sorted(DT)


def _vector(dt, seed=0):
    rng = np.random.default_rng(seed)
    mag = 10.0 ** rng.uniform(-6, 3, N)
    if dt == "f16":
        mag[: N // 10] = 2.0 ** rng.uniform(-24, -14, N // 10)
    return mag * rng.choice([-1.0, 1.0], N)


def _rne(x, dt):
    """float64 -> the format, one round to nearest even (torch converts a double directly), as a 16-bit tensor."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(DT[dt])


def _f64(t):
    return t.double().numpy()


def _bands(key):
    """Index sets of the decades of |key| (1e-8 .. 1e4): one call each."""
    dec = np.floor(np.log10(np.maximum(np.abs(key), 1e-300))).astype(int)
    return [np.flatnonzero(dec == d) for d in range(-9, 5) if (dec == d).any()]


def _caught(got, want, dt, key=None):
    """(largest ratio, fraction of all elements outside the bar), decade by decade."""
    worst, n_out = 0.0, 0
    for idx in _bands(want if key is None else key):
        worst = max(worst, SC.ratio(got[idx], want[idx], dt))
        n_out += SC.over(got[idx], want[idx], dt) * idx.size
    return worst, n_out / want.size


def _toward_zero(x, dt):
    """Truncation: the neighbour of the format towards zero (sign-magnitude patterns: one less is one step towards zero)."""
    r = _rne(x, dt)
    too_big = np.abs(_f64(r)) > np.abs(x)
    b = SC.bits(r).copy()
    b[too_big] -= 1
    return torch.from_numpy(b).view(DT[dt])


@pytest.mark.parametrize("dt", TYPES)
def test_one_rounding_of_the_truth_stays_inside_the_bar(dt):
    want = _vector(dt)
    got = _f64(_rne(want, dt))
    worst, frac = _caught(got, want, dt)
    whole = SC.ratio(got, want, dt)
    print("reference %s: largest ratio per decade %.4f, as one call %.4f" % (dt, worst, whole))
    assert worst <= 1.0 and frac == 0.0 and whole <= 1.0
    assert SC.ratio(got, want, dt, scale=0.0) <= 1.0                # even with no absolute term at all
    assert worst > 0.9                                              # ... and the bar is not slack: the worst element nearly fills it


@pytest.mark.parametrize("dt", TYPES)
def test_truncation_is_caught(dt):
    want = _vector(dt, 1)
    worst, frac = _caught(_f64(_toward_zero(want, dt)), want, dt)
    print("truncation %s: ratio %.3f, outside %.1f %%" % (dt, worst, 100 * frac))
    assert worst > 1.0 and frac >= 0.10


def _ties(dt, seed=2):
    """Exact midpoints a + ulp/2 of adjacent numbers of the format (exact in float32 too: p + 1 bits), a of both signs, even and odd."""
    a = _f64(_rne(_vector(dt, seed), dt))
    a = a[np.abs(a) >= 2.0 ** SC.FORMATS[dt][1]]                    # normal numbers
    return a, a + np.sign(a) * 0.5 * SC.ulp16(a, dt)


@pytest.mark.parametrize("dt", TYPES)
def test_round_half_away_is_invisible_to_the_bar_and_caught_bit_for_bit(dt):
    a, tie = _ties(dt)
    assert np.array_equal(tie.astype(np.float32).astype(np.float64), tie)
    right = _rne(tie, dt)
    away = _rne(a + np.sign(a) * SC.ulp16(a, dt), dt)               # always the neighbour away from zero
    a_even = (SC.bits(_rne(a, dt)) & 1) == 0                        # a even: nearest-even stays at a, away-from-zero leaves it
    assert np.array_equal(_f64(right)[~a_even], _f64(away)[~a_even])
    worst, _ = _caught(_f64(away), tie, dt)
    assert worst <= 1.0                                             # half an ulp off, like the right answer
    frac = SC.mismatch(away, right)
    print("half away %s: ratio %.3f, bit mismatches %.1f %%" % (dt, worst, 100 * frac))
    assert frac >= 0.10 and abs(frac - a_even.mean()) < 1e-12
    assert SC.mismatch(right, _rne(tie.astype(np.float32), dt)) == 0.0


@pytest.mark.parametrize("dt", TYPES)
def test_two_roundings_are_caught(dt):
    x = _vector(dt, 3)
    f = 1.0 + 2.0 ** -5
    want = x * f
    mid = _rne(x, dt).float() * np.float32(f)                       # round, multiply in float32, round again
    got = _f64(mid.to(DT[dt]))
    worst, frac = _caught(got, want, dt)
    print("two roundings %s: ratio %.3f, outside %.1f %%" % (dt, worst, 100 * frac))
    assert worst > 1.0 and frac >= 0.10
    once = _f64((torch.from_numpy(x).float() * np.float32(f)).to(DT[dt]))       # the same in float32, rounded once: inside
    assert _caught(once, want, dt)[0] <= 1.0


@pytest.mark.parametrize("dt", TYPES)
def test_a_sixteen_bit_partial_sum_is_caught(dt):
    """27 taps -- the cubic B-spline at a lattice point, (1/6, 2/3, 1/6)^3 -- of random stored data."""
    rng = np.random.default_rng(4)
    w1 = np.array([1.0, 4.0, 1.0]) / 6.0
    w = np.einsum("i,j,k->ijk", w1, w1, w1).reshape(-1)
    mag = _vector(dt, 4)
    data = _f64(_rne(rng.standard_normal((N, 27)) * np.abs(mag)[:, None], dt))  # the stored inputs
    want = data @ w
    w32 = torch.from_numpy(w).float()
    d32 = torch.from_numpy(data).float()
    acc16 = torch.zeros(N, dtype=DT[dt])
    acc32 = torch.zeros(N, dtype=torch.float32)
    for k in range(27):
        acc16 = (acc16.float() + w32[k] * d32[:, k]).to(DT[dt])
        acc32 = acc32 + w32[k] * d32[:, k]
    worst, frac = _caught(_f64(acc16), want, dt, key=mag)
    print("16-bit partial sum %s: ratio %.3f, outside %.1f %%" % (dt, worst, 100 * frac))
    assert worst > 1.0 and frac >= 0.10
    assert _caught(_f64(acc32.to(DT[dt])), want, dt, key=mag)[0] <= 1.0         # float32 sum, rounded once: inside


def test_flushed_f16_subnormals_are_caught():
    rng = np.random.default_rng(5)
    want = 2.0 ** rng.uniform(-24, -14, N) * rng.choice([-1.0, 1.0], N)
    kept = _f64(_rne(want, "f16"))
    assert SC.ratio(kept, want, "f16") <= 1.0
    flushed = np.where(np.abs(kept) < 2.0 ** -14, 0.0, kept)
    frac = SC.over(flushed, want, "f16")
    print("flushed subnormals: ratio %.3f, outside %.1f %%" % (SC.ratio(flushed, want, "f16"), 100 * frac))
    assert SC.ratio(flushed, want, "f16") > 1.0 and frac >= 0.10


@pytest.mark.parametrize("dt", TYPES)
def test_ulp16_is_the_distance_to_the_next_number_of_the_format(dt):
    """Every non-negative finite pattern: normal, subnormal, zero, powers of two."""
    top = {"bf16": 0x7F7F, "f16": 0x7BFF}[dt]
    pat = torch.arange(0, top + 1, dtype=torch.int32).to(torch.int16)
    v = pat.view(DT[dt]).double().numpy()
    assert np.all(np.diff(v) > 0)
    assert np.array_equal(SC.ulp16(v[:-1], dt), np.diff(v))
    assert np.array_equal(SC.ulp16(-v[:-1], dt), np.diff(v))
    p, emin = SC.FORMATS[dt]
    assert SC.ulp16(0.0, dt) == 2.0 ** (emin - p + 1) == v[1]
    for k in (emin, -3, 0, 5):
        assert SC.ulp16(2.0 ** k, dt) == 2.0 ** (k - p + 1)
        assert SC.ulp16(np.nextafter(2.0 ** k, 0.0), dt) == 2.0 ** (max(k - 1, emin) - p + 1)
    assert SC.ulp16(2.0 ** -24, "f16") == 2.0 ** -24 and SC.ulp16(2.0 ** -15, "f16") == 2.0 ** -24
    assert SC.name(torch.bfloat16) == "bf16" and SC.name(torch.float16) == "f16"


def test_the_bar_as_the_issue_states_it():
    want = np.array([1.0, -3.0, 1e-3, 0.0])
    e = 1e-5 * np.abs(want) + 1e-5 * 3.0
    e7 = 1e-5 * np.abs(want) + 1e-5 * 7.0
    for dt in TYPES:
        assert np.array_equal(SC.bar(want, dt), 0.5 * SC.ulp16(np.abs(want) + e, dt) + e)
        assert np.array_equal(SC.bar(want, dt, scale=7.0), 0.5 * SC.ulp16(np.abs(want) + e7, dt) + e7)
    assert SC.ratio(np.array([np.nan]), np.array([1.0]), "f16") == np.inf
    assert np.array_equal(SC.f32_bar(want), e)
