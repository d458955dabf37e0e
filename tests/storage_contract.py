"""TEST INFRASTRUCTURE ONLY -- the bar of the 16-bit storage contract ("float32 math, rounded once"), in numpy / float64.

A kernel that widens its bf16 / f16 inputs exactly, computes in float32 and rounds its result to nearest even ONCE is off the float64
truth of the stored inputs by at most half a unit in the last place of the format at the float32 result, plus the error of the float32
arithmetic.  The project's float32 kernels are held to  e32 = 1e-5 |want| + 1e-5 max|want|  (tests/golden_util.py: fp32_tol), so

    bar(want) = 0.5 ulp16(|want| + e32) + e32                   elementwise

The half ulp comes from the number format, e32 from the float32 bar the suite already asserts; nothing is taken from the code under test.
`want` is always float64 truth computed from the STORED inputs (rounded to the 16-bit type, then widened), never a kernel's output.

What the bar cannot see: a tie rounded to the wrong neighbour is half an ulp off like the right one.  Rounding DIRECTION at ties is
held bit for bit (`bits` / `mismatch`), on constructed ties where the float32 result is the exact midpoint of two adjacent numbers.

    ulp16(x, dtype)                 spacing of the format at |x|
    bar(want, dtype, scale)         the bar above, scale = max|want| of the call
    ratio(got, want, dtype, scale)  max |got - want| / bar        (<= 1: inside)
    over(got, want, dtype, scale)   fraction of the elements outside the bar
    ulps(got, want, dtype)          max |got - want| / ulp16(|want| + e32): the error in spacings of the format (for the record)
    f32_bar / f32_ratio             the plain float32 bar, for the float32 outputs of a 16-bit call (grid gradients)

`python tests/storage_contract.py < log` condenses the "STORAGE ..." lines that tests/test_storage_contract_gpu.py prints under -s into
the table of profiles/storage_contract.txt."""
import sys

import numpy as np

# precision p (bits of the significand, the hidden one included) and the smallest exponent of a normal number
FORMATS = {"bf16": (8, -126), "f16": (11, -14)}
F16_MAX = 65504.0                 # the largest finite f16; truth at or beyond 65520 = F16_MAX + half an ulp rounds to inf
F16_INF_FROM = 65520.0


def name(dtype):
    """'bf16' / 'f16' for a torch dtype, a numpy dtype or a name."""
    s = str(dtype)
    if s in FORMATS:
        return s
    if "bfloat16" in s:
        return "bf16"
    if "float16" in s or s == "half":
        return "f16"
    raise ValueError("not a 16-bit storage type: %r" % (dtype,))


def ulp16(x, dtype):
    """2^(floor(log2|x|) - (p - 1)) with the exponent floored at the smallest normal one (below it the spacing is constant:
    2^-24 for f16, 2^-133 for bf16), as float64.  |x| = 0 has the subnormal spacing."""
    p, emin = FORMATS[name(dtype)]
    a = np.abs(np.asarray(x, dtype=np.float64))
    _, ex = np.frexp(a)                                   # a = m 2^ex, 0.5 <= m < 1: floor(log2 a) = ex - 1, exactly
    e = np.where(a > 0, ex - 1, emin)
    e = np.maximum(e, emin)
    return np.ldexp(1.0, e - (p - 1))


def e32(want, scale):
    return 1e-5 * np.abs(np.asarray(want, dtype=np.float64)) + 1e-5 * float(scale)


def _scale(want, scale):
    want = np.asarray(want, dtype=np.float64)
    if scale is not None:
        return float(scale)
    return float(np.abs(want).max()) if want.size else 0.0


def bar(want, dtype, scale=None):
    want = np.asarray(want, dtype=np.float64)
    e = e32(want, _scale(want, scale))
    return 0.5 * ulp16(np.abs(want) + e, dtype) + e


def _err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - want)
    return np.where(np.isnan(err), np.inf, err)           # a NaN is outside every bar


def ratio(got, want, dtype, scale=None):
    want = np.asarray(want, dtype=np.float64)
    if want.size == 0:
        return 0.0
    return float((_err(got, want) / bar(want, dtype, scale)).max())


def over(got, want, dtype, scale=None):
    want = np.asarray(want, dtype=np.float64)
    return float((_err(got, want) > bar(want, dtype, scale)).mean())


def ulps(got, want, dtype, scale=None):
    """The largest error in spacings of the format, the spacing taken where the bar takes it: at |want| + e32 (at |want| itself an
    element that cancels to nearly zero would count its float32 error in spacings of a number it is not)."""
    want = np.asarray(want, dtype=np.float64)
    if want.size == 0:
        return 0.0
    return float((_err(got, want) / ulp16(np.abs(want) + e32(want, _scale(want, scale)), dtype)).max())


def f32_bar(want, scale=None):
    want = np.asarray(want, dtype=np.float64)
    return e32(want, _scale(want, scale))


def f32_ratio(got, want, scale=None):
    want = np.asarray(want, dtype=np.float64)
    if want.size == 0:
        return 0.0
    b = f32_bar(want, scale)
    err = _err(got, want)
    return float(np.where(err == 0, 0.0, err / np.maximum(b, 1e-300)).max())


def bits(t):
    """The 16-bit patterns of a torch bf16 / f16 tensor, as a numpy int16 array."""
    import torch
    return t.detach().contiguous().cpu().view(torch.int16).numpy()


def mismatch(got, want):
    """Fraction of the elements of two 16-bit tensors whose bit patterns differ."""
    return float((bits(got) != bits(want)).mean())


def main():
    best = {}
    for line in sys.stdin:
        f = line[line.find("STORAGE"):].split()           # (under -s the line follows pytest's progress dots)
        if len(f) == 6 and f[0] == "STORAGE":
            key = (f[1], f[2], f[3])
            r, u = best.get(key, (0.0, 0.0))
            best[key] = (max(r, float(f[4])), max(u, float(f[5])))
    print("%-26s %-18s %-5s %-14s %s" % ("route", "operator", "type", "largest ratio", "largest error / ulp16"))
    for key in sorted(best):
        print("%-26s %-18s %-5s %-14.3f %.3f" % (key + best[key]))


if __name__ == "__main__":
    main()
