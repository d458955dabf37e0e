"""Composition of displacement fields and scaling-and-squaring, composed route against fused route.

Workload: 1 x n^3 x 3 float32 (n = 256), bound dft, extrapolate; `left` = `right` = one field (a squaring step), either
smooth (a few low Fourier modes, amplitude 2 voxels) or rough (i.i.d. normal, sigma = 2 voxels); orders 1 and 3.

  composed : right + grid_pull(left.movedim(-1, 1), right, displacement=True).movedim(1, -1) through the public API --
             what a commit without `interpol.compose` offers, so it runs on any commit;
  fused    : interpol.compose / interpol.exp (csrc/compose.hip); reported as null on a commit that lacks them.

Measured per (field, order): the forward alone (no_grad), forward + backward to both fields, and exp(steps=8) forward
(no_grad; composed: the same loop over the composed expression).
Method: one process, 5 warm-up steps, then `--steps` (>= 20) steps, each timed with a pair of events; median and the
10th / 90th percentiles are printed.  One JSON line per (route, field, order).  `--route composed|fused|both`, `--n`,
`--orders`, `--all-orders-fused` (by default `interpol.backend.fused_compose_orders` decides which orders the fused route
really runs fused: the others are the composed route under another name).
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


def composed(left, right, **kw):
    return right + interpol.grid_pull(left.movedim(-1, 1), right, displacement=True, **kw).movedim(1, -1)


def exp_composed(vel, steps, **kw):
    u = vel * 2.0 ** -steps
    for _ in range(steps):
        u = composed(u, u, **kw)
    return u


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


def smooth_field(n, amp, gen, dev):
    ax = torch.arange(n, dtype=torch.float32, device=dev) / n
    g = torch.meshgrid(ax, ax, ax, indexing="ij")
    v = torch.zeros([n, n, n, 3], device=dev)
    for d in range(3):
        for _ in range(4):
            k = torch.randint(1, 3, [3], generator=gen)
            ph = 2 * math.pi * float(torch.rand([], generator=gen))
            v[..., d] += torch.sin(2 * math.pi * (float(k[0]) * g[0] + float(k[1]) * g[1] + float(k[2]) * g[2]) + ph)
    return (v * (amp / float(v.abs().max())))[None]


def measure(route, field, order, steps, warmup):
    kw = dict(interpolation=order, bound="dft", extrapolate=True)
    if route == "fused":
        comp = lambda l, r: interpol.compose(l, r, **kw)
        exp8 = lambda v: interpol.exp(v, 8, **kw)
    else:
        comp = lambda l, r: composed(l, r, **kw)
        exp8 = lambda v: exp_composed(v, 8, **kw)
    gy = torch.ones_like(field)

    def fwd():
        with torch.no_grad():
            comp(field, field)

    def fwd_bwd():
        l, r = field.detach().requires_grad_(), field.detach().requires_grad_()
        torch.autograd.grad(comp(l, r), (l, r), gy)

    def exp_fwd():
        with torch.no_grad():
            exp8(field)

    return dict(forward_ms=timed(fwd, steps, warmup), forward_backward_ms=timed(fwd_bwd, steps, warmup),
                exp8_forward_ms=timed(exp_fwd, steps, warmup))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", default="both", choices=["composed", "fused", "both"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--orders", type=int, nargs="+", default=[1, 3])
    ap.add_argument("--all-orders-fused", action="store_true",
                    help="send orders 2 and 3 to the fused kernel too (interpol.backend.fused_compose_orders = (1, 2, 3))")
    a = ap.parse_args()
    if a.all_orders_fused:
        interpol.backend.fused_compose_orders = (1, 2, 3)
    if a.steps < 20:
        ap.error("--steps must be at least 20 (median of at least 20 steps)")
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(0)
    fields = dict(smooth=smooth_field(a.n, 2.0, gen, dev),
                  rough=(2.0 * torch.randn([1, a.n, a.n, a.n, 3], generator=gen)).to(dev))
    have = hasattr(interpol, "compose") and hasattr(interpol, "exp")
    for name, field in fields.items():
        for order in a.orders:
            for route in (("composed", "fused") if a.route == "both" else (a.route,)):
                head = dict(route=route, field=name, order=order, shape=list(field.shape), steps=a.steps,
                            package=os.path.relpath(PKG, ROOT))
                if route == "fused" and not have:
                    print(json.dumps(dict(head, forward_ms=None, note="this commit has no interpol.compose")), flush=True)
                    continue
                print(json.dumps(dict(head, **measure(route, field, order, a.steps, a.warmup))), flush=True)


if __name__ == "__main__":
    main()
