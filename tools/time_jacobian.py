"""Jacobian and Jacobian determinant of a displacement field at its lattice points, composed route against fused route.

Workloads: 1 x n^3 x 3 (n = 256) and 32 x m^2 x 2 (m = 1024), float32, bound dft; the field is either smooth (a few low
Fourier modes, amplitude 2 voxels) or rough (i.i.d. normal, sigma = 2 voxels); orders 1, 2 and 3.

  composed : grid_grad(u.movedim(-1, 1), zeros_like(u), displacement=True).movedim(1, -2) + eye(D), and torch.linalg.det of it,
             through the public API -- what a commit without `interpol.jacobian` offers, so it runs on any commit
             (`--composed` = `--route composed`);
  fused    : interpol.jacobian / interpol.jacdet (csrc/jacobian.hip); reported as null on a commit that lacks them.

Measured per (shape, field, order): `jacobian` forward and `jacdet` forward (no_grad), and `jacdet` forward + backward.
Method: one process, 5 warm-up steps, then `--steps` (>= 20) steps, each timed with a pair of events; median and the
10th / 90th percentiles are printed.  One JSON line per (route, shape, field, order).  The fused lines also carry the
rate of the bytes the operation has to move (the byte model: the field read once, the result written once) in GB/s.
`--all-orders-fused`: by default `interpol.backend.fused_jacobian_orders` decides which orders the fused route really runs
fused (the others are the composed route under another name).
"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.abspath(os.environ.get("INTERPOL_PKG") or os.path.join(ROOT, "torch-interpol_amd"))      # (another checkout's package: A/B across commits)
sys.path.insert(0, PKG)
import interpol  # noqa: E402


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(round(q * (len(v) - 1))))]


def stats(v):
    return dict(median=round(pct(v, 0.5), 4), p10=round(pct(v, 0.1), 4), p90=round(pct(v, 0.9), 4))


def jacobian_composed(u, **kw):
    dim = u.shape[-1]
    J = interpol.grid_grad(u.movedim(-1, 1), torch.zeros_like(u), displacement=True, extrapolate=True, **kw).movedim(1, -2)
    return J + torch.eye(dim, dtype=u.dtype, device=u.device)


def jacdet_composed(u, **kw):
    return torch.linalg.det(jacobian_composed(u, **kw))


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


def measure(route, field, order, steps, warmup):
    kw = dict(interpolation=order, bound="dft")
    if route == "fused":
        jac = lambda u: interpol.jacobian(u, **kw)
        det = lambda u: interpol.jacdet(u, **kw)
    else:
        jac = lambda u: jacobian_composed(u, **kw)
        det = lambda u: jacdet_composed(u, **kw)
    gy = torch.ones(field.shape[:-1], dtype=field.dtype, device=field.device)

    def jac_fwd():
        with torch.no_grad():
            jac(field)

    def det_fwd():
        with torch.no_grad():
            det(field)

    def det_fwd_bwd():
        u = field.detach().requires_grad_()
        torch.autograd.grad(det(u), u, gy)

    res = dict(jacobian_forward_ms=timed(jac_fwd, steps, warmup), jacdet_forward_ms=timed(det_fwd, steps, warmup),
               jacdet_forward_backward_ms=timed(det_fwd_bwd, steps, warmup))
    if route == "fused":
        # the byte model: D components read and D * D (1) written per lattice point
        dim, es, pts = field.shape[-1], field.element_size(), field.numel() // field.shape[-1]
        res["jacobian_forward_GBps"] = round(pts * es * (dim + dim * dim) / res["jacobian_forward_ms"]["median"] / 1e6, 1)
        res["jacdet_forward_GBps"] = round(pts * es * (dim + 1) / res["jacdet_forward_ms"]["median"] / 1e6, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", default="both", choices=["composed", "fused", "both"])
    ap.add_argument("--composed", action="store_true", help="the composed route only (API of any commit): --route composed")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n", type=int, default=256, help="edge of the 3-D lattice, 1 x n^3 x 3 (0: skip)")
    ap.add_argument("--m", type=int, default=1024, help="edge of the 2-D lattices, 32 x m^2 x 2 (0: skip)")
    ap.add_argument("--orders", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--all-orders-fused", action="store_true",
                    help="send every instantiated order to the fused kernels (interpol.backend.fused_jacobian_orders = (1, 2, 3))")
    a = ap.parse_args()
    if a.composed:
        a.route = "composed"
    if a.all_orders_fused:
        interpol.backend.fused_jacobian_orders = (1, 2, 3)
    if a.steps < 20:
        ap.error("--steps must be at least 20 (median of at least 20 steps)")
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(0)
    shapes = ([[1, a.n, a.n, a.n]] if a.n else []) + ([[32, a.m, a.m]] if a.m else [])
    have = hasattr(interpol, "jacobian") and hasattr(interpol, "jacdet")
    for bshape in shapes:
        B, shape = bshape[0], bshape[1:]
        dim = len(shape)
        fields = dict(smooth=torch.stack([smooth_field(shape, 2.0, gen, dev) for _ in range(min(B, 2))])[torch.arange(B) % min(B, 2)].contiguous(),
                      rough=(2.0 * torch.randn([B, *shape, dim], generator=gen)).to(dev))
        for name, field in fields.items():
            for order in a.orders:
                for route in (("composed", "fused") if a.route == "both" else (a.route,)):
                    head = dict(route=route, field=name, order=order, shape=list(field.shape), steps=a.steps,
                                package=os.path.relpath(PKG, ROOT))
                    if route == "fused" and not have:
                        print(json.dumps(dict(head, jacdet_forward_ms=None, note="this commit has no interpol.jacobian")), flush=True)
                        continue
                    if route == "fused":
                        head["fused_orders"] = list(interpol.backend.fused_jacobian_orders)
                    print(json.dumps(dict(head, **measure(route, field, order, a.steps, a.warmup))), flush=True)
        del fields, field
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
