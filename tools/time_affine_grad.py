"""One optimisation step of an affine registration, dense route against fused route.

Workload (config 2's shape): 4 x 2 x 256^3 float32, cubic dct2, extrapolate, one near-identity affine; forward pull plus
backward to the 12 entries of the matrix ONLY (the image needs no gradient).

  dense : grid = affine_grid(mat, shape); y = grid_pull(x, grid); backward through the (B,*shape,3) grid gradient and
          the matmul of affine_grid.  Runs on any commit.
  fused : y = grid_pull(x, AffineGrid(mat, shape)); the backward reduces the grid gradient inside the kernel
          (csrc/affine_grad.hip).  Needs a commit whose AffineGrid is differentiable; reported as null otherwise.

Method: one process, 5 warm-up steps, then `--steps` (>= 20) steps, each timed with a pair of events; median and the
10th / 90th percentiles (the run-to-run spread of one process) are printed, for the whole step and for the backward alone.
One JSON line per route.  `--route dense|fused|both`, `--n` (edge, default 256), `--batch`, `--channels`.
For the per-kernel split run it under `rocprofv3 --kernel-trace --stats -- python tools/time_affine_grad.py --steps 20`.
"""
import argparse
import json
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


def measure(route, x, gy, mat0, shape, steps, warmup):
    kw = dict(interpolation=3, bound="dct2", extrapolate=True)
    total, bwd = [], []
    last = None
    for it in range(warmup + steps):
        mat = mat0.clone().requires_grad_()
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        if route == "dense":
            y = interpol.grid_pull(x, interpol.affine_grid(mat, shape), **kw)
        else:
            y = interpol.grid_pull(x, interpol.AffineGrid(mat, shape), **kw)
        e1.record()
        g, = torch.autograd.grad(y, mat, gy)
        e2.record()
        torch.cuda.synchronize()
        if it >= warmup:
            total.append(e0.elapsed_time(e2))
            bwd.append(e1.elapsed_time(e2))
        last = g
    return dict(route=route, steps=steps, step_ms=dict(median=pct(total, 0.5), p10=pct(total, 0.1), p90=pct(total, 0.9)),
                backward_ms=dict(median=pct(bwd, 0.5), p10=pct(bwd, 0.1), p90=pct(bwd, 0.9)),
                grad_mat=[[float(v) for v in row] for row in last.cpu()])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", default="both", choices=["dense", "fused", "both"])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--channels", type=int, default=2)
    a = ap.parse_args()
    if a.steps < 20:
        ap.error("--steps must be at least 20 (median of at least 20 steps)")
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    shape = (a.n,) * 3
    x = torch.randn([a.batch, a.channels, *shape], generator=g).to(dev)
    gy = torch.randn([a.batch, a.channels, *shape], generator=g).to(dev)
    mat0 = (torch.eye(3, 4) + torch.tensor([[1 / 64, 1 / 128, 0, 0.5], [-1 / 128, -1 / 64, 1 / 256, -0.25],
                                            [0, 1 / 128, 1 / 64, 0.375]])).to(dev)
    fused_ok = True
    try:
        fused_ok = bool(interpol.AffineGrid(mat0.clone().requires_grad_(), shape).requires_grad)
    except Exception:
        fused_ok = False
    for route in (("dense", "fused") if a.route == "both" else (a.route,)):
        if route == "fused" and not fused_ok:
            print(json.dumps(dict(route="fused", step_ms=None, note="this commit's AffineGrid has no gradient")))
            continue
        print(json.dumps(dict(measure(route, x, gy, mat0, shape, a.steps, a.warmup), shape=[a.batch, a.channels, *shape],
                              package=os.path.relpath(PKG, ROOT))), flush=True)


if __name__ == "__main__":
    main()
