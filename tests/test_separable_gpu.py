"""The separable passes (csrc/resample1d.hip) against float64 truth: `_hip.resample1d` and `_SepPush` / `_SepPull` compared with the
dense pass matrix W of tests/separable_truth.py (the oracle's 1-D pull of the indicator channels; forward = x @ W.T, adjoint = y @ W),
at the shapes where `resample1d_adj_gather` takes its rarely taken branches: a restriction by 8 (several rounds of AW stencils, more
than MAXC samples per lattice point), workgroups that walk several slices, several column groups, the hand-over to the scattering
kernel.  tests/test_separable_truth_cpu.py pins, without a GPU, that each shape reaches the branch it is here for.

Bars: float64 1e-11 of max|ref|; float32 the project's rtol 1e-5 + 1e-5 max|ref|; bf16 / f16 (forward only: one pass, one rounding) half
an ulp of the format + the float32 bar (tests/storage_contract.py) against W applied to the rounded input.  Every case prints `PARITY ...` (its largest error over
max|ref|): `python tests/separable_truth.py` condenses a `-s` log into profiles/separable_parity.txt."""
import numpy as np
import pytest
import torch

import golden_util as G
import separable_truth as ST
import storage_contract as SC
from interpol import _hip, separable

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = {"f32": torch.float32, "f64": torch.float64, "bf16": torch.bfloat16, "f16": torch.float16}
_W, _X = {}, {}


def _matrix(kind, ns, nl, dt, bound, order, ex):
    """(lin as the kernel reads it, W): computed once per case, shared, never modified."""
    key = (kind, ns, nl, dt == "f64", bound, order, ex)
    if key not in _W:
        lin = ST.case_lin(kind, ns, nl, dt)
        W = ST.pass_matrix(lin, nl, bound, order, ex)
        W.setflags(write=False)
        _W[key] = (lin, W)
    return _W[key]


def _input(shape, dt, seed=0):
    """The input as stored in `dt` (CPU tensor) and the same values in float64 numpy."""
    key = (tuple(shape), dt, seed)
    if key in _X:
        return _X[key]
    x = torch.randn(list(shape), generator=torch.Generator().manual_seed(seed + len(shape)), dtype=torch.float64).to(DT[dt])
    out = (x, x.double().numpy())
    if x.numel() <= 1 << 22:
        _X[key] = out
    return out


def _put(t, misalign=0):
    """`t` on the device, its first element `misalign` elements past a 256-byte boundary."""
    buf = torch.empty(t.numel() + 260, dtype=t.dtype, device=DEV)
    off = (-(buf.data_ptr() // t.element_size()) % (256 // t.element_size())) + misalign
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 256 == misalign * t.element_size() and v.is_contiguous()
    return v


def _lin(lin, dt):
    return torch.from_numpy(lin).to(torch.float64 if dt == "f64" else torch.float32).to(DEV)


def _close(got, want, dt, org, order, what):
    got = got.detach().double().cpu().numpy()
    print("PARITY separable %s %s %d %.3e" % (org, dt, order, G.rel_err(got, want)))
    if dt == "f64":
        assert G.rel_err(got, want) < 1e-11, (what, G.rel_err(got, want))
    elif dt == "f32":
        G.assert_close(got, want, rtol=1e-5, atol_rel=1e-5, what=str(what))
    else:
        r = SC.ratio(got, want, dt)
        assert r <= 1.0, (what, r)


def _gathers(dt, ns, inner):
    return bool(_hip.lib().interpol_resample_1d_gathers(_hip._DTYPE_CODE[DT[dt]], ns, inner))


def _adjoint(xd, lin, dim, order, bound, ex, nl):
    return _hip.resample1d(xd, lin, dim, order, bound, ex, ST.iso_mode(order), adjoint=True, n_lattice=nl)


# ---------------------------------------------------------------------------
# adjoint, LASTDIM (inner == 1): x (outer, 1100) -> 137
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("outer,kind,order,dt,bound,ex", ST.lastdim_cases(),
                         ids=lambda v: str(v))
def test_adjoint_gather_last_dim(outer, kind, order, dt, bound, ex):
    lin, W = _matrix(kind, ST.NS, ST.NL, dt, bound, order, ex)
    x, x64 = _input((outer, ST.NS), dt)
    assert _gathers(dt, ST.NS, 1)
    xd, ld = _put(x), _lin(lin, dt)
    got = _adjoint(xd, ld, -1, order, bound, ex, ST.NL)
    assert got.shape == (outer, ST.NL) and got.dtype == DT[dt]
    _close(got, ST.apply_adjoint(x64, W, -1), dt, "adj_gather_lastdim", order, (outer, kind, order, dt, bound, ex))
    assert torch.equal(got, _adjoint(xd, ld, -1, order, bound, ex, ST.NL))          # no atomics: bit-identical


# ---------------------------------------------------------------------------
# adjoint, lanes along the columns: x (outer, ns, inner) -> nl
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,outer,ns,inner,nl,misalign,kind,order,dt,bound,ex", ST.column_cases(),
                         ids=lambda v: str(v))
def test_adjoint_gather_columns(name, outer, ns, inner, nl, misalign, kind, order, dt, bound, ex):
    vec = ST.is_vec(inner, dt, misalign)
    if outer is None:                           # the smallest number of slices that makes a workgroup walk UB + 1 of them
        outer = ST.smallest_outer_for_chunk(ns, inner, nl, ST.UB + 1, vec)
    lin, W = _matrix(kind, ns, nl, dt, bound, order, ex)
    x, x64 = _input((outer, ns, inner), dt)
    assert _gathers(dt, ns, inner)
    xd, ld = _put(x, misalign), _lin(lin, dt)
    got = _adjoint(xd, ld, 1, order, bound, ex, nl)
    assert got.shape == (outer, nl, inner) and got.dtype == DT[dt]
    if name in ("vec4", "cgroups2052", "chunk5"):       # the float4 path is taken on 16-byte aligned bases only
        assert xd.data_ptr() % 16 == 0 and got.data_ptr() % 16 == 0 and inner % 4 == 0
    if name == "off16":
        assert xd.data_ptr() % 16 != 0 and inner % 4 == 0
    _close(got, ST.apply_adjoint(x64, W, 1), dt, "adj_gather_" + name, order, (name, outer, kind, order, dt, bound, ex))
    assert torch.equal(got, _adjoint(xd, ld, 1, order, bound, ex, nl))


# ---------------------------------------------------------------------------
# the hand-over to the scattering kernel (atomics into a zero-filled target)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape,nl,gathered,kind,order,dt,bound,ex", ST.handover_cases(), ids=lambda v: str(v))
def test_adjoint_hand_over_to_the_scattering_kernel(shape, nl, gathered, kind, order, dt, bound, ex):
    ns, inner = shape[1], (shape[2] if len(shape) == 3 else 1)
    lin, W = _matrix(kind, ns, nl, dt, bound, order, ex)
    x, x64 = _input(shape, dt)
    xd, ld = _put(x), _lin(lin, dt)
    got = _adjoint(xd, ld, 1, order, bound, ex, nl)
    assert _gathers(dt, ns, inner) == gathered
    org = "adj_gather_4096" if gathered else ("adj_atomics_4097" if inner == 1 else "adj_atomics_inner8")
    _close(got, ST.apply_adjoint(x64, W, 1), dt, org, order, (shape, kind, order, dt, bound, ex))
    if gathered:
        assert torch.equal(got, _adjoint(xd, ld, 1, order, bound, ex, nl))


# ---------------------------------------------------------------------------
# forward: f32 (float4 and scalar), f64, bf16, f16
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,shape,dim,misalign,ns,dt,order,kind,bound,ex", ST.forward_cases(), ids=lambda v: str(v))
def test_forward(name, shape, dim, misalign, ns, dt, order, kind, bound, ex):
    nl = shape[dim]
    lin, W = _matrix(kind, ns, nl, dt, bound, order, ex)
    x, x64 = _input(shape, dt)
    xd, ld = _put(x, misalign), _lin(lin, dt)
    got = _hip.resample1d(xd, ld, dim, order, bound, ex, ST.iso_mode(order))
    assert got.dtype == DT[dt] and got.shape == shape[:dim] + (ns,) + shape[dim + 1:]
    if name == "cols64":
        assert xd.data_ptr() % 16 == 0 and got.data_ptr() % 16 == 0
    _close(got, ST.apply_forward(x64, W, dim), dt, "fwd_" + name, order, (name, ns, dt, order, kind, bound, ex))


# ---------------------------------------------------------------------------
# through autograd, D = 3: a restriction by 8 along every dim, and its transpose
# ---------------------------------------------------------------------------
SSHAPE, TSHAPE = (80, 72, 264), (10, 9, 33)


@pytest.mark.parametrize("order,dt,kind,b0,ex", [(o, d, ("affine", "wide")[(i + j) % 2], (3 * i + j) % 7, (i + j) % 3)
                                                  for i, o in enumerate(ST.ORDERS) for j, d in enumerate(("f32", "f64"))])
def test_separable_push_and_pull_through_autograd(order, dt, kind, b0, ex):
    bounds, orders = [b0, (b0 + 3) % 7, (b0 + 5) % 7], [order] * 3
    mats = [_matrix(kind, ns, nl, dt, b, order, ex) for ns, nl, b in zip(SSHAPE, TSHAPE, bounds)]
    lin = [_lin(m[0], dt) for m in mats]

    def push(a):
        for d, m in enumerate(mats):
            a = ST.apply_adjoint(a, m[1], 2 + d)
        return a

    def pull(a):
        for d, m in enumerate(mats):
            a = ST.apply_forward(a, m[1], 2 + d)
        return a
    fine, fine64 = _input((1, 2) + SSHAPE, dt)
    coarse, coarse64 = _input((1, 2) + TSHAPE, dt, seed=1)
    # push, backward = pull
    xd = fine.to(DEV).requires_grad_(True)
    assert separable._gathers(xd, lin)
    y = separable._SepPush.apply(xd, lin, list(TSHAPE), orders, bounds, ex)
    assert y.shape == (1, 2) + TSHAPE
    _close(y, push(fine64), dt, "autograd_push", order, ("push", order, dt, kind, bounds, ex))
    y.backward(coarse.to(DEV))
    _close(xd.grad, pull(coarse64), dt, "autograd_push_bwd", order, ("push backward", order, dt, kind, bounds, ex))
    # pull, backward = push
    vd = coarse.to(DEV).requires_grad_(True)
    z = separable._SepPull.apply(vd, lin, orders, bounds, ex)
    assert z.shape == (1, 2) + SSHAPE
    _close(z, pull(coarse64), dt, "autograd_pull", order, ("pull", order, dt, kind, bounds, ex))
    z.backward(fine.to(DEV))
    _close(vd.grad, push(fine64), dt, "autograd_pull_bwd", order, ("pull backward", order, dt, kind, bounds, ex))
