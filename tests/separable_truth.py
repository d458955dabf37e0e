"""TEST INFRASTRUCTURE ONLY -- the float64 truth of the separable passes (csrc/resample1d.hip) as ONE DENSE MATRIX PER PASS, the
cases that tests/test_separable_gpu.py runs, and the launch / window arithmetic of `resample1d_adj_gather` restated in numpy so that
tests/test_separable_truth_cpu.py can say, without a GPU, which branch of the kernel each case reaches.

    W = pass_matrix(lin, nl, bound, order, extrapolate)        (ns, nl), float64
    forward : y = x @ W.T along the dim          adjoint : x = y @ W along the dim

W is the oracle's 1-D grid_pull of the nl indicator channels: nothing of the library under test takes part in it.

`python tests/separable_truth.py < log` condenses the "PARITY ..." lines that the GPU tests print into the table of
profiles/separable_parity.txt (the largest error per organisation, dtype and order)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:                        # (run as a script; under pytest tests/conftest.py has done it)
    sys.path.insert(0, ROOT)
from oracle import oracle

ORDERS = (0, 1, 3, 5)
KINDS = ("affine", "wide", "runs", "unsorted")
B_DST1 = 4                                      # csrc/spline_math.hpp:22

# ---- constants of resample1d_adj_gather, each with its line in csrc/resample1d.hip (a change there that moves a case off its branch
# fails tests/test_separable_truth_cpu.py)
ADJ_NS_MAX = 4096                               # resample1d.hip:101
AW = {True: 384, False: 64}                     # resample1d.hip:106   stencils resident per round (LASTDIM, not LASTDIM)
LT = {True: 128, False: 4}                      # resample1d.hip:107   lattice points per workgroup
MAXC = {True: 24, False: 64}                    # resample1d.hip:108   (sample, weight) pairs kept per lattice point
UB = 4                                          # resample1d.hip:218   slices in flight per thread
CSPAN_MAX = 8                                   # resample1d.hip:284   column tiles a workgroup walks
NY_THREADS = {True: 1 << 17, False: 1 << 19}    # resample1d.hip:291   threads side by side before a workgroup loops over slices


def iso_mode(order):
    """The iso-mode rule of test_resample1d_passes: iso1 for order 1, iso0 for order 0, else the general stencil."""
    return 1 if order == 1 else (2 if order == 0 else 0)


def round_lin(lin, dtype_name):
    """`lin` as the kernel reads it: float32 for f32 / bf16 / f16 data, float64 for f64 -- returned as float64."""
    lin = np.asarray(lin, dtype=np.float64)
    return lin if dtype_name == "f64" else lin.astype(np.float32).astype(np.float64)


def off_thresholds(lin, nl):
    """Coordinates within 1e-3 of a mask threshold (nd.py:10-27) are moved 4e-3 off it, as `_grid` of tests/test_memory_contract.py
    does and for its reason: float32 and float64 round the threshold differently, so a coordinate ON it is masked by one and not by
    the other.  (The shift is far below the spacing of every lattice used here: a sorted `lin` stays sorted.)"""
    lin = np.array(lin, dtype=np.float64)
    for thr in (-0.55, -0.05, nl - 1 + 0.05, nl - 1 + 0.55):
        near = np.abs(lin - thr) < 1e-3
        lin = np.where(near, lin + 4e-3, lin)
    return lin


def lattice(kind, ns, nl, seed=0):
    """The four lattice kinds of test_separable_push_by_gathering_passes, as float64 numpy."""
    if kind == "affine":
        lin = np.linspace(-0.5, nl - 0.5, ns)
    elif kind == "wide":
        lin = np.linspace(-3.3, nl + 2.6, ns)
    elif kind == "runs":
        lin = np.round(np.linspace(0.2, nl - 1.1, ns))
    elif kind == "unsorted":
        lin = np.linspace(-0.5, nl - 0.5, ns)[np.random.default_rng(seed).permutation(ns)]
    else:
        raise ValueError(kind)
    return off_thresholds(lin, nl)


def pass_matrix(lin, nl, bound, order, extrapolate):
    """(ns, nl) float64 matrix of one pass: oracle.grid_pull of the nl indicator channels at the coordinates `lin`."""
    lin = np.asarray(lin, dtype=np.float64)
    vol = np.eye(nl, dtype=np.float64)[None]                                   # (1, C = nl, nl)
    out = oracle.grid_pull(vol, lin.reshape(1, -1, 1), [int(bound)], [int(order)], int(extrapolate))
    return np.ascontiguousarray(np.asarray(out)[0].T)                          # (ns, nl)


def apply_forward(x, W, dim):
    """x (..., nl, ...) -> (..., ns, ...): x @ W.T along `dim`, float64."""
    x = np.moveaxis(np.asarray(x, dtype=np.float64), dim, -1)
    return np.ascontiguousarray(np.moveaxis(x @ W.T, -1, dim))


def apply_adjoint(y, W, dim):
    """y (..., ns, ...) -> (..., nl, ...): y @ W along `dim`, float64."""
    y = np.moveaxis(np.asarray(y, dtype=np.float64), dim, -1)
    return np.ascontiguousarray(np.moveaxis(y @ W, -1, dim))


# ---------------------------------------------------------------------------
# launch_adj_gather (resample1d.hip:277-294) and the windows of a workgroup (resample1d.hip:130-142), restated
# ---------------------------------------------------------------------------
def gathers(ns, inner):
    """adjoint_gathers, resample1d.hip:274."""
    return ns <= ADJ_NS_MAX and (inner == 1 or inner >= 64)


def launch_geometry(ns, inner, nl, outer, vec):
    last = inner == 1
    ct = 1 if last else (256 if vec else 64)
    ctiles = -(-inner // ct)
    cspan = min(ctiles, CSPAN_MAX)
    cgroups = -(-ctiles // cspan)
    blocks = -(-nl // LT[last]) * cgroups
    slices = -(-outer // 8) if last else outer
    ny = min(NY_THREADS[last] // (blocks * 256) + 1, slices, 65535)
    return dict(last=last, ctiles=ctiles, cspan=cspan, cgroups=cgroups, blocks=blocks, ny=ny, chunk=-(-outer // ny),
                tiles=-(-nl // LT[last]), last_group_tiles=ctiles - (cgroups - 1) * cspan, last_tile_cols=inner - (ctiles - 1) * ct)


def smallest_outer_for_chunk(ns, inner, nl, chunk, vec):
    outer = 1
    while launch_geometry(ns, inner, nl, outer, vec)["chunk"] < chunk:
        outer += 1
    return outer


def windows(lin, nl, order, bound, last):
    """Per lattice tile: (sorted, w0, w1, elo, ehi, total) -- the four bisections of s_range and the length of the virtual list."""
    lin = np.asarray(lin, dtype=np.float64)
    ns, K, h = lin.size, order, 0.5 * (order - 1)
    is_sorted = bool(np.all(lin[:-1] <= lin[1:]))
    lb = lambda v: int(np.searchsorted(lin, v, side="left"))                   # first s with lin[s] >= v
    out = []
    for l0 in range(0, nl, LT[last]):
        if not is_sorted:
            out.append((False, 0, ns, 0, ns, ns))
            continue
        w0, w1 = lb(l0 - K - 1 + h), lb(l0 + LT[last] + 1 + h)
        elo, ehi = lb(h + (2 if bound == B_DST1 else 1)), lb(nl - K - 1 + h)
        ehi = max(ehi, elo)
        out.append((True, w0, w1, elo, ehi, (w1 - w0) + elo + (ns - ehi)))
    return out


def branch_counts(lin, nl, order, bound, extrapolate, last):
    """What decides the branches of one adjoint pass: the largest virtual list of a tile (rounds = ceil(total / AW)), the largest
    number of samples with a non-zero weight on one lattice point, and the largest such number among the MAIN-window entries of ONE
    round of an interior lattice point (the list of a lattice point starts again in every round)."""
    W = pass_matrix(lin, nl, bound, order, extrapolate)
    nz = W != 0
    win = windows(lin, nl, order, bound, last)
    per_round = 0
    for t, (is_sorted, w0, w1, elo, ehi, total) in enumerate(win):
        l0, l1 = t * LT[last], min(nl, (t + 1) * LT[last])
        for v0 in range(0, w1 - w0, AW[last]):
            rows = slice(w0 + v0, min(w1, w0 + v0 + AW[last]))
            per_round = max(per_round, int(nz[rows, l0:l1].sum(0).max()))
    return dict(total=max(w[5] for w in win), rounds=max(-(-w[5] // AW[last]) for w in win), feed=int(nz.sum(0).max()),
                feed_round=per_round, tiles=len(win), sorted=win[0][0])


# ---------------------------------------------------------------------------
# the cases of tests/test_separable_gpu.py
# ---------------------------------------------------------------------------
def rotate(i):
    """bound 0-6 and extrapolate 0-2 of case i of an organisation: 21 consecutive cases meet every pair once."""
    return i % 7, (i // 7 + i) % 3


NS, NL = 1100, 137              # a restriction by 8: two LASTDIM lattice tiles, the second ragged (137 = 128 + 9)
NS_C, NL_C = 300, 37            # the same ratio where the lanes run along the columns


def lastdim_cases():
    """(outer, kind, order, dtype, bound, extrapolate): x (outer, 1100) -> 137."""
    out, i = [], 0
    for outer in (6, 37, 2100):
        for kind in KINDS:
            for order in ORDERS:
                for dt in ("f32", "f64"):
                    if outer == 2100 and dt == "f64" and kind in ("runs", "unsorted"):
                        continue                    # (chunk > 8 is a matter of slices, not of lattice kinds: two kinds in f64)
                    out.append((outer, kind, order, dt) + rotate(i))
                    i += 1
    return out


def column_cases():
    """(name, outer, ns, inner, nl, misalign, kind, order, dtype, bound, extrapolate); outer None: the smallest with chunk >= 5."""
    out, i = [], 0
    shapes = [("vec4", 3, NS_C, 64, NL_C, 0), ("off16", 3, NS_C, 64, NL_C, 1), ("ragged66", 2, NS_C, 66, NL_C, 0),
              ("cgroups577", 2, NS_C, 577, NL_C, 0), ("cgroups2052", 2, NS_C, 2052, NL_C, 0)]
    for name, outer, ns, inner, nl, mis in shapes:
        for kind in KINDS:
            for order in ORDERS:
                for dt in ("f32", "f64"):
                    if name.startswith("cgroups") and kind in ("runs", "unsorted") and dt == "f64":
                        continue
                    out.append((name, outer, ns, inner, nl, mis, kind, order, dt) + rotate(i))
                    i += 1
    for kind, order in (("affine", 3), ("wide", 5), ("runs", 1), ("affine", 0)):
        for dt in ("f32", "f64"):
            if dt == "f64" and order in (0, 1):
                continue
            out.append(("chunk5", None, NS, 64, NL, 0, kind, order, dt) + rotate(i))
            i += 1
    return out


def handover_cases():
    """(shape, nl, gathered, kind, order, dtype, bound, extrapolate): the two sides of ns == ADJ_NS_MAX, and inner in 2..63."""
    out, i = [], 0
    for shape, nl, gathered in (((3, 4096), 512, True), ((3, 4097), 512, False), ((3, 300, 8), 37, False)):
        for kind in ("affine", "wide", "unsorted"):
            for order in ORDERS:
                for dt in ("f32", "f64"):
                    out.append((shape, nl, gathered, kind, order, dt) + rotate(i))
                    i += 1
    return out


def forward_cases():
    """(name, shape, dim, misalign, ns, dtype, order, kind, bound, extrapolate): the eight cases of a (layout, dtype) meet the
    seven bounds."""
    out, i = [], 0
    layouts = (("cols64", (5, 137, 64), 1, 0), ("cols64_off", (5, 137, 64), 1, 1), ("cols66", (5, 137, 66), 1, 0),
               ("cols66_off", (5, 137, 66), 1, 1), ("lastdim", (700, 137), 1, 0))
    for a, (name, shape, dim, misalign) in enumerate(layouts):
        for b, ns in enumerate((1100, 53)):
            for c, dt in enumerate(("f32", "f64", "bf16", "f16")):
                for d, order in enumerate(ORDERS):
                    out.append((name, shape, dim, misalign, ns, dt, order, KINDS[i % 4], (4 * b + d + a + c) % 7, i % 3))
                    i += 1
    return out


def is_vec(inner, dt, misalign):
    return dt == "f32" and inner % 4 == 0 and not misalign


def case_lin(kind, ns, nl, dt):
    return round_lin(lattice(kind, ns, nl, seed=ns + nl), dt)


def main():
    best = {}
    for line in sys.stdin:
        f = line[line.find("PARITY"):].split()                  # (under -s the line follows pytest's progress dots)
        if len(f) == 6 and f[0] == "PARITY":
            key = (f[1], f[2], f[3], int(f[4]))
            best[key] = max(best.get(key, 0.0), float(f[5]))
    print("%-12s %-22s %-5s %-5s %s" % ("file", "organisation", "dtype", "order", "largest error / max|ref|"))
    for key in sorted(best):
        print("%-12s %-22s %-5s %-5d %.3e" % (key + (best[key],)))


if __name__ == "__main__":
    main()
