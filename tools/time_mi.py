"""The mutual-information data term on a dense displacement field (loss, gradient, per-voxel majoriser), composed route against fused.

Workloads, float32, bound dct2, extrapolate = True, ranges None (aminmax on the device); the moving image is i.i.d. normal, the fixed
image a non-monotone function of it plus noise (so that the joint histogram is neither flat nor a line); each on a smooth field (a
low-frequency cosine of amplitude 2 voxels) and on an i.i.d. normal field of sigma = 2 voxels:
  1 x 1 x n^3 (n = 256): orders 1, 2, 3, B = 32 and 64 bins, hessian = 'full' and None;
  32 x 1 x m^2 (m = 1024): orders 1, 2, 3, 32 bins, hessian = 'full'.

  composed : interpol.mi_gauss_newton with `interpol.backend.fused_mi_orders = ()` -- grid_pull and grid_grad at a displacement,
             `index_add_` into a float64 histogram and element-wise passes (interpol/torch_kernels.py: mi_gauss_newton_composed);
  fused    : the same call with every order routed to csrc/mi.hip.

Method: one process; per row the two routes alternate in `--rounds` blocks of `--steps` calls (composed: `--composed-steps`) after
`--warmup` (composed: `--composed-warmup`) warm-up calls each, every call timed with a pair of events (the ranges -- two aminmax --
are part of the call on both routes); the median and the 10th / 90th percentiles of ms per call over all blocks are printed.  One
JSON line per (route, row).  After each row the largest difference between the routes' outputs is printed, relative to the largest
entry of each output.

`--kernel-split` then runs every fused row `--steps` times under torch.profiler and prints the mean device time per call of each
kernel (the per-kernel split; profiling slows the host: never in the timed run).  `--only-fused-case I` (`--only-composed-case I`)
runs row I on that route alone and prints nothing else: the program to put behind a kernel tracer.  `--fused-only` times the fused
route alone (the A/B of two builds of the library, INTERPOL_HIP_LIB).
"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.abspath(os.environ.get("INTERPOL_PKG") or os.path.join(ROOT, "torch-interpol_amd"))
sys.path.insert(0, PKG)
import interpol  # noqa: E402

ALL_ORDERS = (1, 2, 3)
FIELDS = ("smooth", "rough")


def route(orders):
    interpol.backend.fused_mi_orders = orders


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(round(q * (len(v) - 1))))]


def stats(v):
    return dict(median=round(pct(v, 0.5), 4), p10=round(pct(v, 0.1), 4), p90=round(pct(v, 0.9), 4))


def times(fn, steps, warmup):
    ms = []
    for it in range(warmup + steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if it >= warmup:
            ms.append(e0.elapsed_time(e1))
    return ms


def rows(n, m):
    work = []
    if n:
        work += [([1, 1, n, n, n], order, bins, hess, field) for field in FIELDS for order in ALL_ORDERS for bins in (32, 64)
                 for hess in ("full", None)]
    if m:
        work += [([32, 1, m, m], order, 32, "full", field) for field in FIELDS for order in ALL_ORDERS]
    return work


def displacement(kind, B, shape, gen, dev):
    dim = len(shape)
    if kind == "rough":
        return (2.0 * torch.randn([B, *shape, dim], generator=gen)).to(dev)
    o = interpol.identity_grid(shape, device=dev)
    cols = [2.0 * torch.cos(sum(o[..., e] * (2 * math.pi * (1 + (d + e) % 2) / shape[e]) for e in range(dim)) + d) for d in range(dim)]
    return torch.stack(cols, -1).expand(B, *shape, dim).contiguous()


def kernel_split(call, steps):
    """mean device microseconds per call of every kernel, by name (torch.profiler)"""
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(steps):
            call()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.key_averages():
        t = getattr(ev, "device_time_total", None)
        if t is None:
            t = getattr(ev, "cuda_time_total", 0)
        if t:
            out[ev.key.split("(")[0][-60:]] = round(t / steps, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--composed-steps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--composed-warmup", type=int, default=None, help="warm-up calls of the composed route (default: --warmup)")
    ap.add_argument("--n", type=int, default=256, help="edge of the 3-D lattice (0: skip)")
    ap.add_argument("--m", type=int, default=1024, help="edge of the 2-D lattices, 32 x 1 x m^2 (0: skip)")
    ap.add_argument("--kernel-split", action="store_true")
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--cases", type=str, default=None, help="comma-separated row numbers (default: every row)")
    ap.add_argument("--only-fused-case", type=int, default=None)
    ap.add_argument("--only-composed-case", type=int, default=None)
    a = ap.parse_args()
    only = a.only_fused_case if a.only_fused_case is not None else a.only_composed_case
    cwarm = a.warmup if a.composed_warmup is None else a.composed_warmup
    if not torch.cuda.is_available():
        sys.exit("time_mi: needs a GPU (no timing is taken on the CPU)")
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(0)
    work = rows(a.n, a.m)
    if only is not None:
        work = [work[only]]
    elif a.cases:
        work = [work[int(i)] for i in a.cases.split(",")]
    cache = {}
    names = ("fused",) if a.fused_only else ("composed", "fused")
    for bshape, order, bins, hess, kind in work:
        B, shape = bshape[0], bshape[2:]
        key = (tuple(bshape), kind)
        if key not in cache:
            cache.clear()
            interpol.backend.release_workspaces()
            torch.cuda.empty_cache()
            moving = torch.randn([B, 1, *shape], generator=gen).to(dev)
            fixed = torch.cos(2.0 * moving) + 0.25 * torch.randn([B, 1, *shape], generator=gen).to(dev)
            cache[key] = (moving, fixed, displacement(kind, B, shape, gen, dev))
        moving, fixed, disp = cache[key]
        kw = dict(interpolation=order, bound="dct2", extrapolate=True, hessian=hess, bins=bins)
        call = lambda: interpol.mi_gauss_newton(moving, fixed, disp, **kw)
        if only is not None:
            route(ALL_ORDERS if a.only_fused_case is not None else ())
            for _ in range(a.warmup + a.steps):
                call()
            torch.cuda.synchronize()
            return
        ms, out = dict(composed=[], fused=[]), {}
        for rnd in range(a.rounds):                                       # the routes alternate: other work shares the machine
            for name in names:
                route(ALL_ORDERS if name == "fused" else ())
                if name == "fused":
                    ms[name] += times(call, a.steps, a.warmup if rnd == 0 else 1)
                else:
                    ms[name] += times(call, a.composed_steps, cwarm if rnd == 0 else min(cwarm, 1))
                if rnd == 0:
                    out[name] = call()
        row = dict(shape=bshape, field=kind, order=order, bins=bins, hessian=hess)
        for name in names:
            res = dict(route=name, **row, calls=len(ms[name]), call_ms=stats(ms[name]))
            if name == "fused" and not a.fused_only:
                res["speedup_over_composed"] = round(stats(ms["composed"])["median"] / res["call_ms"]["median"], 2)
            print(json.dumps(res), flush=True)
        if not a.fused_only:
            diff = {k: float("%.3g" % float((f.double() - c.double()).abs().max() / c.double().abs().max()))
                    for k, f, c in zip(("loss", "gradient", "hessian"), out["fused"], out["composed"]) if f is not None}
            print(json.dumps(dict(**row, max_difference_fused_composed_over_largest_entry=diff)), flush=True)
        out.clear()
        if a.kernel_split:
            route(ALL_ORDERS)
            try:
                split = kernel_split(call, a.steps)
            except Exception as e:                                        # (no tracer in this session: the timed lines stand alone)
                split = dict(error=repr(e))
            print(json.dumps(dict(**row, kernel_us_per_call=split)), flush=True)


if __name__ == "__main__":
    main()
