"""CPU checks of tests/separable_truth.py: the dense pass matrix W is the oracle's operator (y @ W == oracle.grid_push of the same
line, rows are a partition of unity), and every case of tests/test_separable_gpu.py that is there to reach a branch of
`resample1d_adj_gather` does reach it -- by the kernel's own arithmetic, restated in numpy from the lines of csrc/resample1d.hip
given beside each constant in separable_truth.py.  This is a check of the test INPUTS: if a later change of a constant moves a case
off its branch, this file says so without a GPU."""
import os
import re

import numpy as np
import pytest

import separable_truth as ST
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("order", ST.ORDERS)
@pytest.mark.parametrize("kind", ST.KINDS)
def test_adjoint_of_the_matrix_is_the_oracles_push(kind, order):
    """y @ W == oracle.grid_push of the line, to 1e-12 (measured 1.8e-15 for 1100 -> 137, cubic, dct2)."""
    rng = np.random.default_rng(order)
    for bound in range(7):
        ex = (order + bound) % 3
        lin = ST.lattice(kind, ST.NS, ST.NL, seed=3)
        W = ST.pass_matrix(lin, ST.NL, bound, order, ex)
        assert W.shape == (ST.NS, ST.NL) and W.dtype == np.float64
        y = rng.standard_normal((1, 3, ST.NS))
        want = np.asarray(oracle.grid_push(y, lin.reshape(1, -1, 1), [ST.NL], [bound], [order], ex))
        got = ST.apply_adjoint(y, W, -1)
        err = np.abs(got - want).max() / np.abs(want).max()
        assert err < 1e-12, (kind, order, bound, ex, err)
        x = rng.standard_normal((1, 3, ST.NL))
        want = np.asarray(oracle.grid_pull(x, lin.reshape(1, -1, 1), [bound], [order], ex))
        err = np.abs(ST.apply_forward(x, W, -1) - want).max() / np.abs(want).max()
        assert err < 1e-12, ("forward", kind, order, bound, ex, err)


@pytest.mark.parametrize("order", ST.ORDERS)
def test_rows_sum_to_one_inside_the_lattice(order):
    lin = ST.lattice("wide", ST.NS, ST.NL)
    for bound in range(7):
        for ex in range(3):
            rows = ST.pass_matrix(lin, ST.NL, bound, order, ex).sum(1)
            # the whole stencil inside the lattice, one point clear of its ends (the reference's dst1 gives lattice point 0 the
            # sign of the implicit zero in front of it: a tap there counts nothing): every bound
            deep = (lin >= order + 1) & (lin <= ST.NL - 2 - order)
            assert deep.sum() > ST.NS // 2 and np.abs(rows[deep] - 1).max() < 1e-13, (order, bound, ex)
            # the sample inside the lattice: the bounds that mirror, repeat or wrap the image without changing its sign
            if bound in (1, 2, 3, 6):
                inside = (lin >= 0) & (lin <= ST.NL - 1)
                assert np.abs(rows[inside] - 1).max() < 1e-13, (order, bound, ex)


def test_lin_is_rounded_to_what_the_kernel_reads_and_kept_off_the_mask_thresholds():
    for kind in ST.KINDS:
        l64, l32 = ST.case_lin(kind, ST.NS, ST.NL, "f64"), ST.case_lin(kind, ST.NS, ST.NL, "f32")
        assert np.array_equal(l32, l32.astype(np.float32).astype(np.float64))
        assert np.abs(l64 - l32).max() < 2e-5
        for lin in (l64, l32):
            for thr in (-0.55, -0.05, ST.NL - 1 + 0.05, ST.NL - 1 + 0.55):
                assert np.abs(lin - thr).min() > 9e-4, (kind, thr)
            assert bool(np.all(lin[:-1] <= lin[1:])) == (kind != "unsorted")


def test_the_constants_are_those_of_the_kernel():
    """The constants restated in separable_truth.py, read back from the lines of csrc/resample1d.hip that define them."""
    src = open(os.path.join(ROOT, "torch-interpol_amd", "csrc", "resample1d.hip")).read()

    def one(pattern):
        m = re.search(pattern, src)
        assert m, pattern
        return tuple(int(g) for g in m.groups())
    assert one(r"constexpr int ADJ_NS_MAX = (\d+);") == (ST.ADJ_NS_MAX,)
    assert one(r"constexpr int AW = LASTDIM \? (\d+) : (\d+);") == (ST.AW[True], ST.AW[False])
    assert one(r"constexpr int LT = LASTDIM \? (\d+) : (\d+),") == (ST.LT[True], ST.LT[False])
    assert one(r"constexpr int MAXC = LASTDIM \? (\d+) : (\d+),") == (ST.MAXC[True], ST.MAXC[False])
    assert one(r"constexpr int UB = (\d+);") == (ST.UB,)
    assert one(r"const int cspan = ctiles < (\d+) \? ctiles : (\d+);") == (ST.CSPAN_MAX, ST.CSPAN_MAX)
    assert one(r"\(last \? 1u << (\d+) : 1u << (\d+)\)") == (17, 19)
    assert (ST.NY_THREADS[True], ST.NY_THREADS[False]) == (1 << 17, 1 << 19)


def test_lastdim_cases_reach_their_branches():
    """x (outer, 1100) -> 137: two lattice tiles, the second ragged; more than one round of AW = 384 stencils (resample1d.hip:106)
    for every sorted lattice; orders 3 and 5 feed a lattice point from more than MAXC = 24 samples (resample1d.hip:108), inside ONE
    round too; outer = 2100 makes a workgroup take more than the 2 x UB = 8 slices of one step (resample1d.hip:218-228)."""
    cases = ST.lastdim_cases()
    assert {c[4] for c in cases} == set(range(7)) and {c[5] for c in cases} == {0, 1, 2}
    assert {(c[1], c[2], c[3]) for c in cases if c[0] == 6} == {(k, o, d) for k in ST.KINDS for o in ST.ORDERS for d in ("f32", "f64")}
    seen = set()
    for outer, kind, order, dt, bound, ex in cases:
        geo = ST.launch_geometry(ST.NS, 1, ST.NL, outer, False)
        assert ST.gathers(ST.NS, 1) and geo["last"] and geo["tiles"] == 2 and ST.NL % ST.LT[True] != 0
        if outer == 2100:
            assert geo["chunk"] > 2 * ST.UB and geo["chunk"] % (2 * ST.UB) != 0, geo       # a second step, cut short by b >= bend
        else:
            assert geo["chunk"] <= 2 * ST.UB
        if outer == 37:
            assert outer % 2 == 1
        if outer != 6:
            continue                                                                    # (the lattice does not depend on outer)
        bc = ST.branch_counts(ST.case_lin(kind, ST.NS, ST.NL, dt), ST.NL, order, bound, ex, True)
        assert bc["sorted"] == (kind != "unsorted")
        assert bc["total"] > ST.AW[True] and bc["rounds"] >= 2, (kind, order, bc)
        if kind in ("affine", "wide"):
            assert bc["rounds"] >= 3, (kind, order, bc)
        if order in (3, 5) and kind != "runs":          # (runs: see below)
            assert bc["feed"] > ST.MAXC[True], (kind, order, bc)
            if kind != "unsorted":
                assert bc["feed_round"] > ST.MAXC[True], (kind, order, bc)
        seen.add((kind, order, bc["feed"] > ST.MAXC[True]))
    # `runs` puts its samples ON the lattice points: B-spline weights at integer offsets, K - 1 non-zero taps -- fewer feeders
    # than `affine`, still more than MAXC at order 5
    assert ("runs", 5, True) in seen


def test_column_cases_reach_their_branches():
    """Lanes along the columns (LT = 4 lattice points, AW = 64 stencils per round, resample1d.hip:106-107): a restriction by 8 needs
    several rounds at every order; 577 scalar columns and 2052 float4 columns need two column groups, the last one partial
    (resample1d.hip:283-285); the `chunk5` cases make a workgroup walk 5 slices, one more than the UB = 4 in flight."""
    cases = ST.column_cases()
    assert {c[9] for c in cases} == set(range(7)) and {c[10] for c in cases} == {0, 1, 2}
    names = {c[0] for c in cases}
    assert names == {"vec4", "off16", "ragged66", "cgroups577", "cgroups2052", "chunk5"}
    done = set()
    for name, outer, ns, inner, nl, mis, kind, order, dt, bound, ex in cases:
        vec = ST.is_vec(inner, dt, mis)
        if outer is None:
            outer = ST.smallest_outer_for_chunk(ns, inner, nl, ST.UB + 1, vec)
            assert outer * ns * inner * 8 < 200e6                                       # (bytes of the float64 case)
        geo = ST.launch_geometry(ns, inner, nl, outer, vec)
        assert ST.gathers(ns, inner) and not geo["last"]
        if name == "vec4":
            assert vec == (dt == "f32") and geo["cgroups"] == 1 and geo["chunk"] == 1
        if name == "off16":
            assert not vec and inner % 4 == 0
        if name == "ragged66":
            assert geo["ctiles"] == 2 and geo["last_tile_cols"] == 2 and not vec
        if name == "cgroups577":
            assert geo["cgroups"] >= 2 and geo["last_group_tiles"] < geo["cspan"] and geo["last_tile_cols"] == 1 and not vec
        if name == "cgroups2052":
            assert geo["cgroups"] >= 2 and geo["last_group_tiles"] < geo["cspan"] and vec == (dt == "f32")
        if name == "chunk5":
            assert geo["chunk"] >= ST.UB + 1 and geo["chunk"] % ST.UB != 0, geo
        key = (ns, nl, kind, order, dt, bound, ex)
        if key in done:
            continue
        done.add(key)
        bc = ST.branch_counts(ST.case_lin(kind, ns, nl, dt), nl, order, bound, ex, False)
        if kind != "unsorted" and order >= 1:
            assert bc["total"] > ST.AW[False] and bc["rounds"] >= 2, (name, kind, order, bc)
        if kind == "unsorted":
            assert bc["total"] == ns > ST.AW[False]


def test_hand_over_shapes_sit_on_the_rule():
    assert ST.gathers(4096, 1) and not ST.gathers(4097, 1)
    assert ST.gathers(300, 64) and not ST.gathers(300, 8) and not ST.gathers(300, 63) and not ST.gathers(300, 2)


def test_forward_and_hand_over_cases_meet_every_bound():
    seen = {(c[0], c[5], c[8]) for c in ST.forward_cases()}
    layouts = ("cols64", "cols64_off", "cols66", "cols66_off", "lastdim")
    assert seen == {(n, d, b) for n in layouts for d in ("f32", "f64", "bf16", "f16") for b in range(7)}
    assert {c[9] for c in ST.forward_cases()} == {0, 1, 2}
    for shape in ((3, 4096), (3, 4097), (3, 300, 8)):
        mine = [c for c in ST.handover_cases() if c[0] == shape]
        assert {c[6] for c in mine} == set(range(7)) and {c[7] for c in mine} == {0, 1, 2}
        ns, inner = shape[1], (shape[2] if len(shape) == 3 else 1)
        assert all(c[2] == ST.gathers(ns, inner) for c in mine)
