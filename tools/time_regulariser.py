"""The displacement-field regulariser (absolute / membrane / bending), composed route against fused route.

Workloads: 1 x n^3 x 3 (n = 256) with bounds dft and dct2, and 32 x m^2 x 2 (m = 1024) with dft, float32; the field is either
smooth (a few low Fourier modes, amplitude 2 voxels) or rough (i.i.d. normal, sigma = 2 voxels); weights: membrane only,
bending only, all three.

  composed : interpol.regulariser / regulariser_energy with `interpol.backend.fused_regulariser = False` -- one index_select pass
             per tap through the bound tables (interpol/torch_kernels.py), what a user writes without the kernels;
  fused    : the same calls with the backend switch on (csrc/regulariser.hip: one thread per lattice point);
  tile     : (only with a library built by `make experiments`, INTERPOL_HIP_LIB=.../libinterpol_hip_exp.so) the LDS halo tile
             of experiments/regulariser_tile.inc, 3-D float32 L v only; its result is compared with the fused one first.

Measured per (shape, bound, field, weights): `regulariser` forward and `regulariser_energy` forward (no_grad), and
`regulariser_energy` forward + backward.  Method: one process, `--warmup` warm-up steps, then `--steps` (>= 20; the composed
route: `--composed-steps`) steps, each timed with a pair of events; median and the 10th / 90th percentiles are printed.  One
JSON line per (route, shape, bound, field, weights).  The fused lines also carry the time of the byte model (the field read
once, L v written once: 8 D bytes per lattice point; the energy: 4 D) at the measured copy rate of 6.29 TB/s and the
fraction of it that was reached.
"""
import argparse
import ctypes
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.abspath(os.environ.get("INTERPOL_PKG") or os.path.join(ROOT, "torch-interpol_amd"))
sys.path.insert(0, PKG)
import interpol  # noqa: E402
from interpol import _hip  # noqa: E402

COPY_TBPS = 6.29
WEIGHTS = dict(membrane=dict(membrane=1.0), bending=dict(bending=1.0), all=dict(absolute=0.3, membrane=0.7, bending=1.3))


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(round(q * (len(v) - 1))))]


def stats(v):
    return dict(median=round(pct(v, 0.5), 4), p10=round(pct(v, 0.1), 4), p90=round(pct(v, 0.9), 4))


def timed(fn, steps, warmup):
    ms = []
    for it in range(warmup + steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if it >= warmup:
            ms.append(e0.elapsed_time(e1))
    return stats(ms)


def smooth_field(shape, amp, gen, dev):
    dim = len(shape)
    g = torch.meshgrid(*[torch.arange(n, dtype=torch.float32, device=dev) / n for n in shape], indexing="ij")
    v = torch.zeros([*shape, dim], device=dev)
    for d in range(dim):
        for _ in range(4):
            k = torch.randint(1, 3, [dim], generator=gen)
            ph = 2 * math.pi * float(torch.rand([], generator=gen))
            v[..., d] += torch.sin(2 * math.pi * sum(float(k[e]) * g[e] for e in range(dim)) + ph)
    return v * (amp / float(v.abs().max()))


def tile_entry():
    """interpol_regulariser_tile of a library built with the experiments, or None"""
    try:
        fn = _hip.lib().interpol_regulariser_tile
    except AttributeError:
        return None
    fn.argtypes = list(_hip.lib().interpol_regulariser.argtypes)
    fn.restype = ctypes.c_int
    return fn


def tile_call(fn, field, weights, bound, out):
    dim = field.shape[-1]
    p = _hip._regulariser_problem(field, [interpol.codes.bound_to_code(bound)] * dim, out.stride(0))
    a, m, b, vx = _hip._regulariser_weights(weights, [1.0] * dim, dim)
    rc = fn(ctypes.byref(p), _hip._ptr(field), _hip._ptr(out), a, m, b, vx, _hip._stream(field.device))
    if rc:
        raise RuntimeError("interpol_regulariser_tile: %d" % rc)
    return out


def measure(field, bound, w, steps, warmup):
    kw = dict(bound=bound, **w)
    gy = torch.ones(field.shape[0], dtype=field.dtype, device=field.device)

    def matvec():
        with torch.no_grad():
            interpol.regulariser(field, **kw)

    def energy():
        with torch.no_grad():
            interpol.regulariser_energy(field, **kw)

    def energy_fwd_bwd():
        u = field.detach().requires_grad_()
        torch.autograd.grad(interpol.regulariser_energy(u, **kw), u, gy)

    return dict(matvec_ms=timed(matvec, steps, warmup), energy_ms=timed(energy, steps, warmup),
                energy_forward_backward_ms=timed(energy_fwd_bwd, steps, warmup))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", default="both", choices=["composed", "fused", "both"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--composed-steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n", type=int, default=256, help="edge of the 3-D lattice, 1 x n^3 x 3 (0: skip)")
    ap.add_argument("--m", type=int, default=1024, help="edge of the 2-D lattices, 32 x m^2 x 2 (0: skip)")
    ap.add_argument("--weights", nargs="+", default=list(WEIGHTS), choices=list(WEIGHTS))
    a = ap.parse_args()
    if a.steps < 20:
        ap.error("--steps must be at least 20 (median of at least 20 steps)")
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(0)
    tile = tile_entry()
    work = ([([1, a.n, a.n, a.n], b) for b in ("dft", "dct2")] if a.n else []) + ([([32, a.m, a.m], "dft")] if a.m else [])
    fields, last = {}, None
    for bshape, bound in work:
        B, shape = bshape[0], bshape[1:]
        dim = len(shape)
        if last != bshape:
            fields.clear()
            torch.cuda.empty_cache()
            fields.update(smooth=torch.stack([smooth_field(shape, 2.0, gen, dev) for _ in range(min(B, 2))])[torch.arange(B) % min(B, 2)].contiguous(),
                          rough=(2.0 * torch.randn([B, *shape, dim], generator=gen)).to(dev))
            last = bshape
        for name, field in fields.items():
            for wname in a.weights:
                w = WEIGHTS[wname]
                for route in (("composed", "fused") if a.route == "both" else (a.route,)):
                    interpol.backend.fused_regulariser = route == "fused"
                    head = dict(route=route, shape=list(field.shape), bound=bound, field=name, weights=wname,
                                steps=a.steps if route == "fused" else a.composed_steps)
                    res = measure(field, bound, w, head["steps"], a.warmup if route == "fused" else 2)
                    if route == "fused":
                        pts = field.numel() // dim
                        for key, nbytes in (("matvec", 8 * dim), ("energy", 4 * dim)):
                            model = pts * nbytes / (COPY_TBPS * 1e12) * 1e3
                            res[key + "_model_ms"] = round(model, 4)
                            res[key + "_fraction_of_model"] = round(model / res[key + "_ms"]["median"], 3)
                    print(json.dumps(dict(head, **res)), flush=True)
                interpol.backend.fused_regulariser = True
                if tile is not None and dim == 3:
                    weights = (w.get("absolute", 0.), w.get("membrane", 0.), w.get("bending", 0.))
                    ref = interpol.regulariser(field, bound=bound, **w)
                    out = torch.empty_like(field)
                    tile_call(tile, field, weights, bound, out)
                    # the two kernels order their sums differently: the difference is held against the terms that are summed,
                    # 2^-24 times the absolute coefficients of a row (unit voxels: absolute + 12 membrane + 144 bending) times max|v|
                    scale = 2.0 ** -24 * (weights[0] + 12 * weights[1] + 144 * weights[2]) * float(field.abs().max())
                    err = float((out - ref).abs().max()) / scale
                    res = dict(route="tile", shape=list(field.shape), bound=bound, field=name, weights=wname, steps=a.steps,
                               max_difference_from_fused_in_ulps_of_the_row_sum=round(err, 2),
                               matvec_ms=timed(lambda: tile_call(tile, field, weights, bound, out), a.steps, a.warmup))
                    print(json.dumps(res), flush=True)
                    assert err <= 32, err


if __name__ == "__main__":
    main()
